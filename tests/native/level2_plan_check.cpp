// level2_plan_check.cpp -- the Level-2 range planner (lambda_amd/csrc/lx_level2_plan.h) from the command line, for
// tests/test_level2_plan.py: no device, no library.  Reads one request per line from standard input, answers each with one line:
//   count N RECORDS_ON_DEVICE FORCED NEED_BYTES HAVE_BYTES     -> R
//   need N SLOT_BYTES                                          -> bytes
//   probes N R                                                 -> target:from:upto ...   ("-" where there is none)
//   cuts N Q_FRAMES P target from upto (P times) RUNS count q (RUNS times)  -> the ranges' bounds
//        (the list's windows are given as runs of `count` windows of frame-expanded query id q; the probes' windows are copied out of
//        it into a block of kL2ProbeWindows per probe, exactly as large as the driver's: what l2_cuts reads beyond it, the sanitizer sees)
//   cfg C19 C13 C11                                            -> columns per lane of the strips chosen
//   consts                                                     -> kFpMaxRanges kL2ProbeWindows
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "lx_level2_plan.h"

int main()
{
    std::string line;
    while (std::getline(std::cin, line))
    {
        std::istringstream in(line);
        std::string        what;
        in >> what;
        if (what == "count")
        {
            uint64_t n, rod, forced, need, have;
            in >> n >> rod >> forced >> need >> have;
            printf("%llu\n", (unsigned long long)lxi::l2_range_count(n, rod != 0, forced, need, have));
        }
        else if (what == "need")
        {
            uint64_t n, slot;
            in >> n >> slot;
            printf("%llu\n", (unsigned long long)lxi::l2_slot_need_bytes(n, slot));
        }
        else if (what == "probes")
        {
            uint64_t n, R;
            in >> n >> R;
            auto const probes = lxi::l2_probe_targets(n, R);
            for (auto const & p : probes)
                printf("%llu:%llu:%llu ", (unsigned long long)p.target, (unsigned long long)p.from, (unsigned long long)p.upto);
            printf(probes.empty() ? "-\n" : "\n");
        }
        else if (what == "cuts")
        {
            uint64_t n, qf, np, nruns;
            in >> n >> qf >> np;
            std::vector<lxi::L2Probe> probes(np);
            for (auto & p : probes)
                in >> p.target >> p.from >> p.upto;
            in >> nruns;
            std::vector<uint32_t> q;
            for (uint64_t r = 0; r < nruns; ++r)
            {
                uint64_t count, id;
                in >> count >> id;
                q.insert(q.end(), count, (uint32_t)id);
            }
            if (!in || q.size() != n)
            {
                fprintf(stderr, "cuts: %zu windows given for a list of %llu\n", q.size(), (unsigned long long)n);
                return 2;
            }
            std::vector<lx::L2Window> block(np * lxi::kL2ProbeWindows, lx::L2Window{0xffffffffu, 0, 0, 0});
            for (size_t k = 0; k < np; ++k)
            {
                if (probes[k].upto > n || probes[k].from > probes[k].upto || probes[k].upto - probes[k].from > lxi::kL2ProbeWindows)
                {
                    fprintf(stderr, "cuts: probe %zu is not inside the list or too long\n", k);
                    return 2;
                }
                for (uint64_t w = probes[k].from; w < probes[k].upto; ++w)
                    block[k * lxi::kL2ProbeWindows + (w - probes[k].from)] = lx::L2Window{q[w], 7, w, w + 1};
            }
            for (uint64_t b : lxi::l2_cuts(block.data(), probes, n, (uint32_t)qf))
                printf("%llu ", (unsigned long long)b);
            printf("\n");
        }
        else if (what == "cfg")
        {
            uint64_t c[3];
            in >> c[0] >> c[1] >> c[2];
            printf("%d\n", lxi::l2_choose_cfg(c));
        }
        else if (what == "consts")
            printf("%u %llu\n", lx::kFpMaxRanges, (unsigned long long)lxi::kL2ProbeWindows);
        else if (!what.empty())
        {
            fprintf(stderr, "unknown request '%s'\n", what.c_str());
            return 2;
        }
        if (!in && !what.empty())
        {
            fprintf(stderr, "malformed request '%s'\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
