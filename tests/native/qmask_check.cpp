// qmask_check.cpp -- the query masking rule's host function (lambda_amd/csrc/lx_qmask.h: seg_mask_sequence, and the word functions the
// kernels share with it) on a corpus written by tests/test_query_mask.py, every input, output and workspace in a heap block of its
// exact size: built with AddressSanitizer and UBSan by that test.  Each record is checked three ways: against the mask the corpus
// states (the Python restatement's), against a plain walk over seg_window_score's flags, and the distance bytes against
// dist_from_bytes of the stated mask.
//
// corpus: "LXQM", u32 records; per record u32 W, thr1, thr2, 65 x u32 T, u32 L, L letters, L mask bytes (0 / 1).
// usage: qmask_check corpus.bin      exit 0 = all records agree
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "lx_qmask.h"

namespace qm = lx::qmask;

static bool take(FILE * f, void * p, size_t n)
{
    return n == 0 || fread(p, 1, n, f) == n;
}

int main(int argc, char ** argv)
{
    if (argc != 2)
        return 2;
    FILE * f = fopen(argv[1], "rb");
    char   magic[4];
    uint32_t n = 0;
    if (!f || !take(f, magic, 4) || memcmp(magic, "LXQM", 4) != 0 || !take(f, &n, 4))
        return 2;
    int bad = 0;
    for (uint32_t r = 0; r < n; ++r)
    {
        qm::SegTables t{};
        uint32_t      W = 0, L = 0;
        if (!take(f, &W, 4) || !take(f, &t.thr1, 4) || !take(f, &t.thr2, 4) || !take(f, t.T, sizeof(t.T)) || !take(f, &L, 4))
            return 2;
        t.W = (int32_t)W;
        std::unique_ptr<uint8_t[]> res(new uint8_t[L]), want(new uint8_t[L]), dist(new uint8_t[L]), plain(new uint8_t[L]), wantDist(new uint8_t[L]);
        if (!take(f, res.get(), L) || !take(f, want.get(), L))
            return 2;
        size_t const                words = (L + 63) / 64;
        std::unique_ptr<uint64_t[]> A(new uint64_t[words]), B(new uint64_t[words]), F(new uint64_t[words]);
        uint64_t const              masked = qm::seg_mask_sequence(res.get(), L, t, dist.get(), A.get(), B.get(), F.get());
        // the plain walk: flags per window from the shared score, runs left to right
        memset(plain.get(), 0, L);
        if (L >= W)
        {
            uint32_t const    nWin = L - W + 1;
            std::vector<char> a(nWin), b(nWin);
            for (uint32_t p = 0; p < nWin; ++p)
            {
                uint32_t const S = qm::seg_window_score(res.get() + p, t.W, t.T);
                a[p] = S >= t.thr2, b[p] = S >= t.thr1;
            }
            for (uint32_t p = 0; p < nWin;)
            {
                if (!a[p])
                {
                    ++p;
                    continue;
                }
                uint32_t e = p;
                bool     trig = b[p];
                while (e + 1 < nWin && a[e + 1])
                {
                    ++e;
                    trig = trig || b[e];
                }
                if (trig)
                    memset(plain.get() + p, 1, e + W - p);
                p = e + 1;
            }
        }
        uint64_t const wantMasked = qm::dist_from_bytes(want.get(), L, wantDist.get());
        bool           ok         = masked == wantMasked;
        for (uint32_t j = 0; j < L && ok; ++j)
            ok = (dist[j] == 0) == (want[j] != 0) && plain[j] == want[j] && dist[j] == wantDist[j];
        if (!ok)
        {
            fprintf(stderr, "record %u (W %u, L %u): the mask differs\n", r, W, L);
            ++bad;
        }
    }
    fclose(f);
    printf("%u records, %d differ\n", n, bad);
    return bad ? 1 : 0;
}
