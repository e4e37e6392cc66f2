// lx_numfmt.h -- the decimal text glibc's printf writes for a double, made with integer arithmetic only; host and device.
//
// The text record kernels (lx_text.hip) must write the bytes the host writer's snprintf calls write (host/lx_output.cpp: "%.1e" of the
// e-value, "%.1f" of the bit score, "%.2f" of pident / ppos, "%g" of SAM's ae), for every value.  No double operation is made here
// beyond taking the bits apart, and no printf: the value is m * 2^e exactly, held in 32-bit limbs, and its decimal digits are peeled
// nine at a time -- the integer part by dividing by 10^9 (the digits come lowest first: the two highest chunks are kept, the rest is
// "anything left"), the fraction by multiplying by 10^9 (the carry out of the top limb is the next nine digits).  Rounding is to
// nearest on the next digits and "anything left", an exact tie to even: glibc's in the default rounding mode.
//
//   kNumE1      "%.1e" of any double: subnormals, +-0, inf / -inf / nan / -nan
//   kNumGFloat  "%g" of a float widened to double (any double is taken; the callers pass (double)(float)x): six significant digits,
//               exponent form below 1e-4 and from 1e6, trailing zeros and a bare point stripped, the exponent at least two digits
//   kNumF1/F2   "%.1f" / "%.2f" of a finite double below 10^15 in magnitude (num_f_domain); others are refused with 0
//
// kNumLimbs limbs: a double's fraction has at most 1074 bits, its integer part at most 1024.  kNumMaxText bounds every text.
#pragma once
#include <cstdint>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace lx
{

enum
{
    kNumE1     = 0,
    kNumF1     = 1,
    kNumF2     = 2,
    kNumGFloat = 3
};
constexpr int      kNumLimbs   = 36;
constexpr int      kNumMaxText = 24; // the longest: "-1234567890123456.78" is outside the F domain; "-999999999999999.99" has 19
constexpr uint32_t kNumE9      = 1000000000u;

__host__ __device__ inline uint64_t num_pow10(int k) // k <= 19
{
    uint64_t p = 1;
    for (int i = 0; i < k; ++i)
        p *= 10;
    return p;
}
__host__ __device__ inline int num_digits(uint64_t v)
{
    int d = 1;
    while (v >= 10)
    {
        v /= 10;
        ++d;
    }
    return d;
}
__host__ __device__ inline int num_put(char * p, uint64_t v, int d) // v in d digits, zero-padded
{
    for (int i = d; i-- > 0;)
    {
        p[i] = (char)('0' + v % 10);
        v /= 10;
    }
    return d;
}

// finite and |v| < 10^15: the domain of the F formats (a comparison of the bits: 10^15 is 0x430c6bf526340000)
__host__ __device__ inline bool num_f_domain(uint64_t bits)
{
    return (bits & 0x7fffffffffffffffull) < 0x430c6bf526340000ull;
}

// the value's exact binary form
struct NumBits
{
    bool     neg;
    int      cls; // 0 zero, 1 finite non-zero, 2 inf, 3 nan
    uint64_t m;   // value = m * 2^e
    int      e;
};
__host__ __device__ inline NumBits num_bits(uint64_t bits)
{
    NumBits        b;
    uint32_t const ex   = (uint32_t)(bits >> 52) & 0x7ffu;
    uint64_t const frac = bits & 0xfffffffffffffull;
    b.neg               = bits >> 63;
    b.m                 = ex ? frac | 1ull << 52 : frac;
    b.e                 = (ex ? (int)ex : 1) - 1075;
    b.cls               = ex == 0x7ff ? (frac ? 3 : 2) : (b.m ? 1 : 0);
    return b;
}

// The fraction F / 2^s (F < 2^s, 1 <= s <= 1074) in kNumLimbs little-endian limbs scaled by 2^(32 kNumLimbs); the limbs below `lo`
// are zero and stay zero under next9.
struct NumFrac
{
    uint32_t w[kNumLimbs];
    int      lo;
    __host__ __device__ void set(uint64_t F, int s)
    {
        for (int i = 0; i < kNumLimbs; ++i)
            w[i] = 0;
        int const      p = 32 * kNumLimbs - s, li = p / 32, sh = p % 32;
        uint64_t const l64 = F << sh, h64 = sh ? F >> (64 - sh) : 0;
        lo                 = li;
        w[li]              = (uint32_t)l64;
        if (li + 1 < kNumLimbs)
            w[li + 1] = (uint32_t)(l64 >> 32);
        if (li + 2 < kNumLimbs)
            w[li + 2] = (uint32_t)h64;
    }
    // the next nine decimal digits
    __host__ __device__ uint32_t next9()
    {
        uint64_t carry = 0;
        for (int i = lo; i < kNumLimbs; ++i)
        {
            uint64_t const t = (uint64_t)w[i] * kNumE9 + carry;
            w[i]             = (uint32_t)t;
            carry            = t >> 32;
        }
        return (uint32_t)carry;
    }
    __host__ __device__ bool any() const
    {
        uint32_t o = 0;
        for (int i = lo; i < kNumLimbs; ++i)
            o |= w[i];
        return o != 0;
    }
};

// The leading digits of a finite non-zero value: `lead` has nd digits (at least 10, or every digit there is), the first of them
// stands for 10^exp10, and `sticky` says whether anything non-zero follows them.
struct NumLead
{
    uint64_t lead;
    int      nd, exp10;
    bool     sticky, exact_short; // exact_short: fewer than 10 digits and nothing follows: zeros may be appended
};
__host__ __device__ inline NumLead num_lead(NumBits const & b)
{
    NumLead r{0, 0, 0, false, false};
    if (b.e >= 0)
    {
        // an integer: m << e, divided by 10^9 until nothing is left
        uint32_t  w[kNumLimbs];
        int const li = b.e / 32, sh = b.e % 32;
        for (int i = 0; i < kNumLimbs; ++i)
            w[i] = 0;
        uint64_t const l64 = b.m << sh, h64 = sh ? b.m >> (64 - sh) : 0;
        w[li]              = (uint32_t)l64; // (e <= 971: li <= 30)
        w[li + 1]          = (uint32_t)(l64 >> 32);
        w[li + 2]          = (uint32_t)h64;
        int      top = li + 2, chunks = 0;
        uint32_t hi = 0, second = 0;
        bool     sticky = false;
        for (;;)
        {
            while (top >= 0 && w[top] == 0)
                --top;
            if (top < 0)
                break;
            uint64_t rem = 0;
            for (int i = top; i >= 0; --i)
            {
                uint64_t const t = rem << 32 | w[i];
                w[i]             = (uint32_t)(t / kNumE9);
                rem              = t % kNumE9;
            }
            sticky = sticky || second != 0;
            second = hi;
            hi     = (uint32_t)rem;
            ++chunks;
        }
        int const nh = num_digits(hi);
        r.exp10      = 9 * (chunks - 1) + nh - 1;
        r.sticky     = sticky;
        if (chunks > 1)
        {
            r.lead = (uint64_t)hi * kNumE9 + second;
            r.nd   = nh + 9;
        }
        else
        {
            r.lead        = hi;
            r.nd          = nh;
            r.exact_short = true;
        }
        return r;
    }
    int const      s = -b.e; // 1 .. 1074
    uint64_t const I = s < 64 ? b.m >> s : 0, F = s < 64 ? b.m & ((1ull << s) - 1) : b.m;
    NumFrac        f;
    f.set(F, s);
    if (I >= kNumE9)
    {
        r.lead   = I;
        r.nd     = num_digits(I);
        r.exp10  = r.nd - 1;
        r.sticky = F != 0;
        return r;
    }
    if (I != 0)
    {
        int const ni = num_digits(I);
        r.lead       = I * kNumE9 + f.next9();
        r.nd         = ni + 9;
        r.exp10      = ni - 1;
        r.sticky     = f.any();
        return r;
    }
    int      j = 1;
    uint32_t c = f.next9();
    while (c == 0) // (F != 0: a non-zero chunk comes, after at most 36 rounds for 2^-1074)
    {
        c = f.next9();
        ++j;
    }
    int const nc = num_digits(c);
    r.lead       = (uint64_t)c * kNumE9 + f.next9();
    r.nd         = nc + 9;
    r.exp10      = -(9 * j - nc + 1);
    r.sticky     = f.any();
    return r;
}

// `lead` rounded to P significant digits (nearest, ties to even); exp10 moves up if the digits carry into a new one
__host__ __device__ inline uint64_t num_round_sig(NumLead r, int P, int & exp10)
{
    exp10 = r.exp10;
    if (r.nd <= P) // (exact_short: every digit is there)
        return r.lead * num_pow10(P - r.nd);
    uint64_t const pw = num_pow10(r.nd - P), half = pw / 2;
    uint64_t       q = r.lead / pw;
    uint64_t const rest = r.lead % pw;
    if (rest > half || (rest == half && (r.sticky || (q & 1))))
        ++q;
    if (q == num_pow10(P))
    {
        q /= 10;
        ++exp10;
    }
    return q;
}

__host__ __device__ inline int num_put_exp(char * o, int x) // e+NN / e-NNN
{
    o[0]           = 'e';
    o[1]           = x < 0 ? '-' : '+';
    uint32_t const a = (uint32_t)(x < 0 ? -x : x);
    int const      d = a >= 100 ? 3 : 2;
    return 2 + num_put(o + 2, a, d);
}

// The text of `bits` (a double's) in format `kind` into out[0 .. kNumMaxText): its length; 0 for an unknown kind or an F value
// outside the domain.  No terminator is written.
__host__ __device__ inline int num_format(int kind, uint64_t bits, char * out)
{
    NumBits const b = num_bits(bits);
    int           n = 0;
    if (kind == kNumF1 || kind == kNumF2)
    {
        if (!num_f_domain(bits))
            return 0;
        int const P = kind == kNumF1 ? 1 : 2;
        uint64_t  I = 0, q = 0;
        if (b.cls == 1)
        {
            int const      s = -b.e; // (positive: a value below 10^15 < 2^52 has a negative e)
            uint64_t const F = s < 64 ? b.m & ((1ull << s) - 1) : b.m;
            I                = s < 64 ? b.m >> s : 0;
            NumFrac f;
            f.set(F, s);
            uint32_t const c  = f.next9();
            uint32_t const pw = (uint32_t)num_pow10(9 - P), half = pw / 2;
            uint32_t const rest = c % pw;
            q                   = c / pw;
            if (rest > half || (rest == half && (f.any() || (q & 1))))
                ++q;
            if (q == num_pow10(P))
            {
                q = 0;
                ++I;
            }
        }
        if (b.neg)
            out[n++] = '-';
        n += num_put(out + n, I, num_digits(I));
        out[n++] = '.';
        n += num_put(out + n, q, P);
        return n;
    }
    if (kind != kNumE1 && kind != kNumGFloat)
        return 0;
    if (b.neg)
        out[n++] = '-';
    if (b.cls >= 2)
    {
        char const * const t = b.cls == 2 ? "inf" : "nan";
        out[n++]             = t[0];
        out[n++]             = t[1];
        out[n++]             = t[2];
        return n;
    }
    int const P = kind == kNumE1 ? 2 : 6;
    uint64_t  q = 0;
    int       x = 0;
    if (b.cls == 1)
        q = num_round_sig(num_lead(b), P, x);
    if (kind == kNumE1)
    {
        out[n++] = (char)('0' + q / 10);
        out[n++] = '.';
        out[n++] = (char)('0' + q % 10);
        return n + num_put_exp(out + n, x);
    }
    // %g: the six digits without their trailing zeros
    char d[6];
    num_put(d, q, 6);
    int nd = 6;
    while (nd > 1 && d[nd - 1] == '0')
        --nd;
    if (b.cls == 0)
    {
        out[n++] = '0';
        return n;
    }
    if (x < -4 || x >= 6)
    {
        out[n++] = d[0];
        if (nd > 1)
        {
            out[n++] = '.';
            for (int i = 1; i < nd; ++i)
                out[n++] = d[i];
        }
        return n + num_put_exp(out + n, x);
    }
    if (x >= 0)
    {
        for (int i = 0; i <= x; ++i) // (digits beyond nd are the stripped zeros)
            out[n++] = d[i];
        if (nd > x + 1)
        {
            out[n++] = '.';
            for (int i = x + 1; i < nd; ++i)
                out[n++] = d[i];
        }
        return n;
    }
    out[n++] = '0';
    out[n++] = '.';
    for (int i = 0; i < -x - 1; ++i)
        out[n++] = '0';
    for (int i = 0; i < nd; ++i)
        out[n++] = d[i];
    return n;
}

} // namespace lx
