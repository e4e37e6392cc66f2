// level3_host_check.cpp -- the host side of Level 3 (include/lambda_ext.h) under the sanitizers, without a device and without Python:
// lx_index_build(NULL, ...), lx_index_save, lx_index_load, lx_index_attach(NULL), lx_seed_queries(NULL, ...) with exact and half-exact
// seeds, the error paths, the free functions.  Build and run on a machine with the library built (no GPU needed):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude tests/native/level3_host_check.cpp
//       -Llambda_amd/csrc -llambda_ext -Wl,-rpath,$PWD/lambda_amd/csrc -o level3_host_check && ASAN_OPTIONS=detect_leaks=0 ./level3_host_check
// (the library itself is the normal build: the sanitizer sees this program, every heap block and every memcpy of the process.)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "lambda_ext.h"

#define CHECK(x)                                                                 \
    do                                                                           \
    {                                                                            \
        if (!(x))                                                                \
        {                                                                        \
            std::fprintf(stderr, "level3 host check: %s failed (line %d): %s\n", #x, __LINE__, lx_last_output_error()); \
            return 1;                                                            \
        }                                                                        \
    } while (0)

int main()
{
    std::mt19937_64       rng(42);
    int const             alph = 10;
    std::vector<uint64_t> sOff, sLen, qOff, qLen;
    std::vector<uint8_t>  sRed, qRed;
    for (int s = 0; s < 25; ++s)
    {
        sOff.push_back(sRed.size());
        sLen.push_back(s == 4 ? 0 : 20 + rng() % 200);
        for (uint64_t i = 0; i < sLen.back(); ++i)
            sRed.push_back((uint8_t)(rng() % alph));
    }
    for (int q = 0; q < 90; ++q) // reads: pieces of subjects and random ones (alignment ranks = reduced letters here)
    {
        qOff.push_back(qRed.size());
        uint64_t const s = rng() % 25, n = 40;
        qLen.push_back(n);
        for (uint64_t i = 0; i < n; ++i)
            qRed.push_back(q % 3 && sLen[s] > n ? sRed[sOff[s] + i] : (uint8_t)(rng() % alph));
    }
    lx_index * ix = nullptr;
    CHECK(lx_index_build(nullptr, sRed.data(), sOff.data(), sLen.data(), sOff.size(), alph, 3, &ix) == LX_OK);
    lx_index_info info{};
    CHECK(lx_index_get_info(ix, &info) == LX_OK && info.key_len == 18 && info.n_entries == sRed.size() && !info.built_on_device);
    std::vector<lx_index_entry> rows(info.n_entries);
    CHECK(lx_index_copy_entries(ix, 0, info.n_entries, rows.data()) == LX_OK);
    for (size_t e = 1; e < rows.size(); ++e)
        CHECK(rows[e - 1].key <= rows[e].key);
    CHECK(lx_index_copy_entries(ix, info.n_entries, 1, rows.data()) == LX_EINVAL);
    lx_bytes * saved = nullptr;
    CHECK(lx_index_save(ix, &saved) == LX_OK && lx_bytes_size(saved) == 32 + 16 * info.n_entries + 8 * info.n_prefix);
    lx_index * back = nullptr;
    for (uint64_t cut : {(uint64_t)0, (uint64_t)31, (uint64_t)32, lx_bytes_size(saved) - 1}) // truncated in every part
        CHECK(lx_index_load(nullptr, lx_bytes_data(saved), cut, sRed.data(), sOff.data(), sLen.data(), sOff.size(), &back) == LX_EINVAL && !back);
    CHECK(lx_index_load(nullptr, lx_bytes_data(saved), lx_bytes_size(saved), sRed.data(), sOff.data(), sLen.data(), sOff.size(), &back) == LX_OK);
    lx_bytes_free(saved);
    lx_index * shared = nullptr;
    CHECK(lx_index_attach(back, nullptr, &shared) == LX_OK);
    lx_index_destroy(back); // (the shared table outlives the index it came from)
    int8_t matrix[LX_ALPH * LX_ALPH];
    for (int a = 0; a < LX_ALPH; ++a)
        for (int b = 0; b < LX_ALPH; ++b)
            matrix[a * LX_ALPH + b] = a == b ? 4 : -2;
    uint64_t counts[2] = {0, 0};
    for (int half = 0; half < 2; ++half)
    {
        lx_seed_params p{};
        p.seed_length = 10, p.seed_offset = 5, p.max_seed_dist = half, p.half_exact = 1, p.adaptive = 1, p.pre_scoring = 2, p.pre_scoring_thresh = 2.0;
        p.max_matches = 256, p.q_num_frames = 1, p.unknown_rank = 25, p.matrix = matrix, p.host_threads = 4;
        lx_seed_result * a = nullptr, * b = nullptr;
        CHECK(lx_seed_queries(nullptr, ix, sRed.data(), qRed.data(), qRed.data(), qOff.data(), qLen.data(), qOff.size(), nullptr, 0, &p, &a) == LX_OK);
        CHECK(lx_seed_queries(nullptr, shared, sRed.data(), qRed.data(), qRed.data(), qOff.data(), qLen.data(), qOff.size(), nullptr, 0, &p, &b) == LX_OK);
        lx_seed_stats const sa = lx_seed_result_stats(a), sb = lx_seed_result_stats(b);
        CHECK(sa.n_matches == sb.n_matches && sa.n_matches > 50 && lx_seed_result_matches_dev(a) == nullptr);
        CHECK(std::memcmp(lx_seed_result_matches(a), lx_seed_result_matches(b), sa.n_matches * sizeof(lx_match)) == 0);
        counts[half] = sa.n_matches;
        uint64_t const bad[1] = {qOff.size()};
        lx_seed_result * none = nullptr;
        CHECK(lx_seed_queries(nullptr, ix, sRed.data(), qRed.data(), qRed.data(), qOff.data(), qLen.data(), qOff.size(), bad, 1, &p, &none) == LX_EINVAL && !none);
        lx_seed_result_free(b);
        lx_seed_result_free(a);
    }
    CHECK(counts[1] >= counts[0]);
    lx_index_destroy(ix);
    lx_index_destroy(shared);
    lx_index_destroy(nullptr);
    lx_seed_result_free(nullptr);
    std::printf("level3 host check: ok (%llu exact, %llu half-exact matches)\n", (unsigned long long)counts[0], (unsigned long long)counts[1]);
    return 0;
}
