// dust_check.cpp -- the nucleotide masking rule's host function (lambda_amd/csrc/lx_dust.h: dust_mask_sequence, and the score functions
// the kernels share with it) on a corpus written by tests/test_query_mask_dust.py, every input and output in a heap block of its
// exact size: built with AddressSanitizer and UBSan by that test.  Each record is checked against the mask the corpus states (the
// Python restatement's), and the distance bytes against dist_from_bytes of the stated mask.  One workspace serves all records, as
// it serves all sequences of a host thread's share.
//
// corpus: "LXDM", u32 records; per record u32 window, level, L, L letters, L mask bytes (0 / 1).
// usage: dust_check corpus.bin      exit 0 = all records agree
#include <cstdio>
#include <cstring>
#include <memory>

#include "lx_dust.h"

namespace qm = lx::qmask;

static bool take(FILE * f, void * p, size_t n)
{
    return n == 0 || fread(p, 1, n, f) == n;
}

int main(int argc, char ** argv)
{
    if (argc != 2)
        return 2;
    FILE *   f = fopen(argv[1], "rb");
    char     magic[4];
    uint32_t n = 0;
    if (!f || !take(f, magic, 4) || memcmp(magic, "LXDM", 4) != 0 || !take(f, &n, 4))
        return 2;
    int          bad = 0;
    qm::DustWork work;
    for (uint32_t r = 0; r < n; ++r)
    {
        uint32_t window = 0, level = 0, L = 0;
        if (!take(f, &window, 4) || !take(f, &level, 4) || !take(f, &L, 4))
            return 2;
        std::unique_ptr<uint8_t[]> res(new uint8_t[L]), want(new uint8_t[L]), dist(new uint8_t[L]), wantDist(new uint8_t[L]);
        if (!take(f, res.get(), L) || !take(f, want.get(), L))
            return 2;
        uint64_t const masked     = qm::dust_mask_sequence(res.get(), L, qm::DustParams{(int32_t)window, (int32_t)level}, dist.get(), work);
        uint64_t const wantMasked = qm::dist_from_bytes(want.get(), L, wantDist.get());
        bool           ok         = masked == wantMasked;
        for (uint32_t j = 0; j < L && ok; ++j)
            ok = dist[j] == wantDist[j];
        if (!ok)
        {
            fprintf(stderr, "record %u (window %u, level %u, L %u): the mask differs\n", r, window, level, L);
            ++bad;
        }
    }
    fclose(f);
    printf("%u records, %d differ\n", n, bad);
    return bad ? 1 : 0;
}
