// fastq_qual_check.cpp -- the FASTQ qualities of the incremental parser (lambda_amd/csrc/host/lx_query_blocks.hpp, keepQualities),
// under AddressSanitizer and UBSan (tests/test_fastq_qual.py builds and runs this).
//
//   fastq_qual_check CORPUS
//
// CORPUS: "LXQB", u32 count, then per input u32 length + bytes.  Per input the text is parsed by RecordParser with the qualities
// kept and with them dropped, each time whole and in pieces of 1, 2, 3 and 7 bytes; every piece is a heap block of its exact size.
// The pieces must give the ids, letters, qualities and error text the whole text gives, a parse that drops the qualities must see
// none (quality() empty while f runs), and a kept quality string is as long as its letters.  Per input: one line
// "<index> K <records> E:<error text>" and the records "R <id>|<letters>|<qualities>" of the parse that keeps them, then
// "<index> D <records> E:<error text>" and "R <id>|<letters>|" of the parse that drops them (bytes outside 0x21..0x7e, "\" and "|"
// as \xx).  Exit status 1 and a line on stderr for the first difference.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "host/lx_query_blocks.hpp"

namespace
{

struct Record
{
    std::string id, letters, qual;
    bool        operator==(Record const & o) const { return id == o.id && letters == o.letters && qual == o.qual; }
};

struct Parse
{
    std::vector<Record> recs;
    std::string         error;
    bool                operator==(Parse const & o) const { return recs == o.recs && error == o.error; }
};

// piece == 0: the whole text at once
Parse parse(std::string const & text, bool keep, size_t piece)
{
    Parse                         out;
    lx_query_blocks::RecordParser parser("reads.fq");
    parser.keepQualities(keep);
    auto f = [&](std::string const & id, std::string & letters)
    {
        out.recs.push_back(Record{id, letters, parser.quality()});
        return true;
    };
    try
    {
        size_t const step = piece ? piece : text.size();
        for (size_t at = 0; at < text.size(); at += step)
        {
            size_t const            n = std::min(step, text.size() - at);
            std::unique_ptr<char[]> block(new char[n]); // (a read past the piece is a read past the block)
            std::memcpy(block.get(), text.data() + at, n);
            parser.feed(block.get(), n, f);
        }
        parser.finish(f);
    }
    catch (std::runtime_error const & e)
    {
        out.error = e.what();
    }
    return out;
}

std::string shown(std::string const & s)
{
    std::string out;
    for (unsigned char c : s)
        if (c < 0x21 || c > 0x7e || c == '\\' || c == '|')
        {
            char buf[8];
            std::snprintf(buf, sizeof(buf), "\\%02x", c);
            out += buf;
        }
        else
            out += (char)c;
    return out;
}

int fail(size_t index, char const * what)
{
    std::fprintf(stderr, "input %zu: %s\n", index, what);
    return 1;
}

} // namespace

int main(int argc, char ** argv)
{
    if (argc != 2)
        return std::fprintf(stderr, "usage: fastq_qual_check CORPUS\n"), 2;
    std::ifstream     in(argv[1], std::ios::binary);
    std::stringstream ss;
    ss << in.rdbuf();
    std::string const corpus = ss.str();
    if (corpus.size() < 8 || corpus.compare(0, 4, "LXQB") != 0)
        return std::fprintf(stderr, "not a corpus\n"), 2;
    uint32_t count = 0;
    std::memcpy(&count, corpus.data() + 4, 4);
    size_t at = 8;
    for (size_t index = 0; index < count; ++index)
    {
        uint32_t len = 0;
        if (at + 4 > corpus.size())
            return std::fprintf(stderr, "corpus cut short\n"), 2;
        std::memcpy(&len, corpus.data() + at, 4);
        if (at + 4 + len > corpus.size())
            return std::fprintf(stderr, "corpus cut short\n"), 2;
        std::string const text = corpus.substr(at + 4, len);
        at += 4 + len;
        for (int keep = 1; keep >= 0; --keep)
        {
            Parse const whole = parse(text, keep != 0, 0);
            for (size_t piece : {1, 2, 3, 7})
                if (!(parse(text, keep != 0, piece) == whole))
                    return fail(index, keep ? "pieces and the whole text differ (qualities kept)" : "pieces and the whole text differ (qualities dropped)");
            for (Record const & r : whole.recs)
            {
                if (!keep && !r.qual.empty())
                    return fail(index, "a quality string although they are dropped");
                if (keep && !r.qual.empty() && r.qual.size() != r.letters.size())
                    return fail(index, "a quality string that is not as long as the letters");
            }
            std::printf("%zu %c %zu E:%s\n", index, keep ? 'K' : 'D', whole.recs.size(), shown(whole.error).c_str());
            for (Record const & r : whole.recs)
                std::printf("R %s|%s|%s\n", shown(r.id).c_str(), shown(r.letters).c_str(), shown(r.qual).c_str());
        }
    }
    return 0;
}
