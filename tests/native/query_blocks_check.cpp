// query_blocks_check.cpp -- the incremental FASTA / FASTQ parser (lambda_amd/csrc/host/lx_query_blocks.hpp) against the whole-text
// rules it replaced, under AddressSanitizer and UBSan (tests/test_query_blocks.py builds and runs this).
//
//   query_blocks_check CORPUS
//
// CORPUS: "LXQB", u32 count, then per input u32 length + bytes.  Per input the text is parsed once by wholeText() -- the front
// end's former forEachRecord, kept here word for word as the yardstick -- and then by RecordParser fed in pieces of 1, 2, 3, 7 and
// 4096 bytes, whole, and in pieces of changing size; every piece is a heap block of its exact size.  Records and error text must
// be equal each time, and so must a parse that the callback stops after its first and after its third record.  Per input one line:
// "<index> <records> <letters> E:<error text>", and the records of the whole-text parse as "R <id>|<letters>" (in all three texts
// bytes outside 0x21..0x7e, "\" and "|" as \xx).  Exit status 1 and a line on stderr for the first difference.
#include <algorithm>
#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "host/lx_query_blocks.hpp"

namespace
{

template <class F>
void wholeText(std::string const & text, std::string const & path, F && f)
{
    size_t       p = 0;
    size_t const n = text.size();
    auto         nextLine = [&](char const *& a, size_t & len) -> bool
    {
        if (p >= n)
            return false;
        size_t e = text.find('\n', p);
        if (e == std::string::npos)
            e = n;
        a   = text.data() + p;
        len = e - p;
        p   = e + 1;
        if (len && a[len - 1] == '\r')
            --len;
        return true;
    };
    auto append = [](std::string & cur, char const * a, size_t len)
    {
        for (size_t i = 0; i < len; ++i)
            if (!std::isspace((unsigned char)a[i]))
                cur.push_back(a[i]);
    };
    size_t const first = text.find_first_not_of(" \t\r\n");
    char const * a     = nullptr;
    size_t       len   = 0;
    std::string  id, cur;
    if (first != std::string::npos && text[first] == '@')
    {
        while (nextLine(a, len))
        {
            if (len == 0)
                continue;
            if (a[0] != '@')
                throw std::runtime_error(path + ": FASTQ record expected, found a line starting with '" + std::string(1, a[0]) + "'");
            id.assign(a + 1, len - 1);
            cur.clear();
            bool plus = false;
            while (nextLine(a, len))
            {
                if (len && a[0] == '+')
                {
                    plus = true;
                    break;
                }
                append(cur, a, len);
            }
            if (!plus)
                throw std::runtime_error(path + ": FASTQ record '" + id + "' has no '+' line");
            size_t quals = 0;
            while (quals < cur.size() && nextLine(a, len))
                quals += len;
            if (quals != cur.size())
                throw std::runtime_error(path + ": FASTQ record '" + id + "' has " + std::to_string(quals) + " quality characters for " +
                                         std::to_string(cur.size()) + " letters");
            if (!f(id, cur))
                return;
        }
        return;
    }
    bool have = false;
    while (nextLine(a, len))
    {
        if (len == 0)
            continue;
        if (a[0] == '>')
        {
            if (have && !f(id, cur))
                return;
            id.assign(a + 1, len - 1);
            cur.clear();
            have = true;
        }
        else if (have)
            append(cur, a, len);
    }
    if (have)
        f(id, cur);
}

struct Parse
{
    std::vector<std::pair<std::string, std::string>> records;
    std::string                                      error;
    bool operator==(Parse const & o) const { return records == o.records && error == o.error; }
};

char const * const kPath = "reads.fq";

// the callback: keeps the record, stops after `stop` records (0 = never)
struct Keep
{
    Parse & r;
    size_t  stop;
    bool operator()(std::string const & id, std::string const & letters)
    {
        r.records.emplace_back(id, letters);
        return r.records.size() != stop;
    }
};

Parse whole(std::string const & text, size_t stop)
{
    Parse r;
    try
    {
        wholeText(text, kPath, Keep{r, stop});
    }
    catch (std::runtime_error const & e)
    {
        r.error = e.what();
    }
    return r;
}

// piece = 0: the whole text in one piece; piece = SIZE_MAX: sizes 1, 5, 2, 11, 3, 64, ... in turn
Parse pieces(std::string const & text, size_t piece, size_t stop)
{
    static size_t const turn[] = {1, 5, 2, 11, 3, 64, 1, 1, 7, 4096};
    Parse r;
    Keep  keep{r, stop};
    try
    {
        lx_query_blocks::RecordParser parser(kPath);
        size_t                        at = 0, t = 0;
        bool                          go = true;
        if (piece == 0)
            go = parser.feed(text.data(), text.size(), keep);
        else
            while (go && at < text.size())
            {
                size_t const      want = piece == SIZE_MAX ? turn[t++ % 10] : piece, n = std::min(want, text.size() - at);
                std::vector<char> block(text.begin() + at, text.begin() + at + n); // (exact size: a read past it is ASan's to find)
                go = parser.feed(block.data(), n, keep);
                at += n;
            }
        if (go)
            parser.finish(keep);
        else if (parser.feed("x", 1, keep) || parser.finish(keep)) // (a stopped parser takes nothing more)
            r.error = "the stopped parser went on";
    }
    catch (std::runtime_error const & e)
    {
        r.error = e.what();
    }
    return r;
}

std::string shown(std::string const & s)
{
    std::string o;
    char        b[8];
    for (unsigned char c : s)
        if (c >= 0x21 && c <= 0x7e && c != '\\' && c != '|')
            o.push_back((char)c);
        else
        {
            snprintf(b, sizeof(b), "\\%02x", c);
            o += b;
        }
    return o;
}

} // namespace

int main(int argc, char ** argv)
{
    // query_blocks_check cutter MAX_READS MAX_LETTERS LEN...: the reads of each block BlockCutter closes, then "open K" for the
    // reads that wait in the last, unclosed one
    if (argc >= 4 && std::strcmp(argv[1], "cutter") == 0)
    {
        lx_query_blocks::BlockCutter cut(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10));
        uint64_t                     in_block = 0;
        for (int i = 4; i < argc; ++i)
        {
            ++in_block;
            if (cut.add(std::strtoull(argv[i], nullptr, 10)))
            {
                if (cut.open())
                    return 1;
                printf("%llu ", (unsigned long long)in_block);
                in_block = 0;
            }
            else if (!cut.open() || cut.reads != in_block)
                return 1;
        }
        printf("open %llu\n", (unsigned long long)in_block);
        return 0;
    }
    if (argc != 2)
        return 2;
    std::ifstream     f(argv[1], std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    std::string const all = ss.str();
    if (all.size() < 8 || all.compare(0, 4, "LXQB") != 0)
        return 2;
    uint32_t count;
    std::memcpy(&count, all.data() + 4, 4);
    size_t at = 8;
    for (uint32_t i = 0; i < count; ++i)
    {
        uint32_t len;
        if (all.size() - at < 4)
            return 2;
        std::memcpy(&len, all.data() + at, 4);
        at += 4;
        if (all.size() - at < len)
            return 2;
        std::string const text = all.substr(at, len);
        at += len;
        for (size_t stop : {(size_t)0, (size_t)1, (size_t)3})
        {
            Parse const want = whole(text, stop);
            for (size_t piece : {(size_t)1, (size_t)2, (size_t)3, (size_t)7, (size_t)4096, (size_t)0, SIZE_MAX})
            {
                Parse const got = pieces(text, piece, stop);
                if (!(got == want))
                {
                    fprintf(stderr, "input %u, pieces of %zu, stop %zu: %zu records, error '%s'; the whole text: %zu records, error '%s'\n", i, piece,
                            stop, got.records.size(), got.error.c_str(), want.records.size(), want.error.c_str());
                    return 1;
                }
            }
            if (stop)
                continue;
            size_t letters = 0;
            for (auto const & r : want.records)
                letters += r.second.size();
            printf("%u %zu %zu E:%s\n", i, want.records.size(), letters, shown(want.error).c_str());
            for (auto const & r : want.records)
                printf("R %s|%s\n", shown(r.first).c_str(), shown(r.second).c_str());
        }
    }
    return 0;
}
