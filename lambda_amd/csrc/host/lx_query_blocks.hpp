// lx_query_blocks.hpp -- the FASTA / FASTQ record rules of the front end as an incremental parser: fed with pieces of any size, it
// gives the records and the error texts the whole text gives.  No HIP and nothing of the library in here: plain C++.
//
// The rules (they were forEachRecord's, which now feeds the whole text to this parser):
//   * lines end at "\n"; a "\r" in front of it is dropped; a last line needs no "\n";
//   * the format comes from the first byte that is none of " \t\r\n": "@" = FASTQ, everything else FASTA;
//   * FASTA: empty lines are skipped, a line starting with ">" begins a record (the id is the rest of the line), every other line
//     adds its non-blank characters to the record; lines in front of the first ">" are ignored;
//   * FASTQ: empty lines between records are skipped; the "@" line, sequence lines up to a line starting with "+", then quality
//     lines until there are as many quality characters as letters -- so a quality line may begin with "@", "+" or ">" --; the
//     qualities are only counted and dropped, as the reference drops them (src/search_algo.hpp:342), unless the parser was told to
//     keep them (keepQualities): then the record's quality string is the bytes of its quality lines as they stand (the "\r" before
//     "\n" dropped as for every line), it is there (quality()) while f runs, and a byte outside '!' .. '~' is refused with the file's
//     path, the record's id and the byte.  The count rule is the same either way, and so are the records and the other error texts.
//     A FASTA text has no qualities: quality() is empty.
// What is carried from piece to piece: the unfinished line, the unfinished record, FASTQ's count of quality characters and, when
// they are kept, the characters.
#pragma once
#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

namespace lx_query_blocks
{

class RecordParser
{
public:
    explicit RecordParser(std::string path) : path_(std::move(path)) {}

    // keep the FASTQ records' qualities (before the first feed)
    void keepQualities(bool keep) { keepQual_ = keep; }
    // while f runs: the record's quality string, as long as its letters -- empty when they are not kept, and for a FASTA record.  f may
    // take it away, like the letters
    std::string & quality() { return qual_; }

    // the next piece of the text.  f(id, letters) per finished record (it may take `letters` away); false once f returned false:
    // the parser has stopped and takes nothing more.  Throws std::runtime_error for a malformed FASTQ record.
    template <class F>
    bool feed(char const * p, size_t n, F && f)
    {
        if (stopped_)
            return false;
        if (!detected_)
            for (size_t i = 0; i < n; ++i)
                if (!std::strchr(" \t\r\n", p[i]) || p[i] == 0)
                {
                    detected_ = true;
                    fastq_    = p[i] == '@';
                    if (fastq_ && blankLine_)
                        notARecord(blankLine_);
                    break;
                }
        while (n)
        {
            char const * const nl = static_cast<char const *>(std::memchr(p, '\n', n));
            if (!nl)
            {
                carry_.append(p, n);
                break;
            }
            size_t const len = (size_t)(nl - p);
            bool         go;
            if (carry_.empty())
                go = line(p, len, f);
            else
            {
                carry_.append(p, len);
                line_.swap(carry_); // (line() may not see carry_ change under it)
                carry_.clear();
                go = line(line_.data(), line_.size(), f);
            }
            if (!go)
                return !(stopped_ = true);
            p += len + 1;
            n -= len + 1;
        }
        return true;
    }

    // the end of the text: the last line if it had no "\n", the last record, the errors of a record cut short
    template <class F>
    bool finish(F && f)
    {
        if (stopped_)
            return false;
        stopped_ = true;
        if (!carry_.empty())
        {
            line_.swap(carry_);
            carry_.clear();
            if (!line(line_.data(), line_.size(), f))
                return false;
        }
        if (fastq_)
        {
            if (state_ == Sequence)
                throw std::runtime_error(path_ + ": FASTQ record '" + id_ + "' has no '+' line");
            if (state_ == Quality)
                badQuality();
            return true;
        }
        if (have_)
            return f(id_, cur_);
        return true;
    }

private:
    enum State
    {
        Header,   // FASTQ: a "@" line comes next
        Sequence, // ... sequence lines, up to the "+" line
        Quality   // ... quality lines, until there are as many characters as letters
    };

    [[noreturn]] void notARecord(char c) const
    {
        throw std::runtime_error(path_ + ": FASTQ record expected, found a line starting with '" + std::string(1, c) + "'");
    }
    [[noreturn]] void badQuality() const
    {
        throw std::runtime_error(path_ + ": FASTQ record '" + id_ + "' has " + std::to_string(quals_) + " quality characters for " +
                                 std::to_string(cur_.size()) + " letters");
    }
    // a quality line joins the record's string (only when the qualities are kept)
    void appendQuality(char const * a, size_t len)
    {
        for (size_t i = 0; i < len; ++i)
            if (a[i] < '!' || a[i] > '~')
            {
                char hex[8];
                std::snprintf(hex, sizeof(hex), "0x%02x", (unsigned)(unsigned char)a[i]);
                throw std::runtime_error(path_ + ": FASTQ record '" + id_ + "' has the byte " + hex + " among its qualities (they are '!' .. '~')");
            }
        qual_.append(a, len);
    }
    void append(char const * a, size_t len)
    {
        for (size_t i = 0; i < len; ++i)
            if (!std::isspace((unsigned char)a[i]))
                cur_.push_back(a[i]);
    }

    // one line, without its "\n"; false: f has stopped the parse
    template <class F>
    bool line(char const * a, size_t len, F && f)
    {
        if (len && a[len - 1] == '\r')
            --len;
        if (!detected_) // (a line of blanks in front of the first record: FASTQ refuses it, once the format is known)
        {
            if (len && !blankLine_)
                blankLine_ = a[0];
            return true;
        }
        if (!fastq_)
        {
            if (len == 0)
                return true;
            if (a[0] == '>')
            {
                if (have_ && !f(id_, cur_))
                    return false;
                id_.assign(a + 1, len - 1);
                cur_.clear();
                have_ = true;
            }
            else if (have_)
                append(a, len);
            return true;
        }
        switch (state_)
        {
        case Header:
            if (len == 0)
                return true;
            if (a[0] != '@')
                notARecord(a[0]);
            id_.assign(a + 1, len - 1);
            cur_.clear();
            state_ = Sequence;
            return true;
        case Sequence:
            if (!(len && a[0] == '+'))
            {
                append(a, len);
                return true;
            }
            quals_ = 0;
            qual_.clear();
            state_ = Quality;
            break;
        case Quality:
            quals_ += len;
            if (keepQual_)
                appendQuality(a, len);
            break;
        }
        if (quals_ < cur_.size())
            return true;
        if (quals_ != cur_.size())
            badQuality();
        state_ = Header;
        return f(id_, cur_);
    }

    std::string path_, carry_, line_, id_, cur_, qual_;
    bool        detected_ = false, fastq_ = false, have_ = false, stopped_ = false, keepQual_ = false;
    char        blankLine_ = 0; // the first character of the first non-empty line seen before the format was known
    State       state_ = Header;
    size_t      quals_ = 0;
};

// Where a block of reads ends: after maxReads reads, or once it holds maxLetters letters (a file of contigs stays bounded).
constexpr uint64_t kBlockLetters = 1ull << 30;

struct BlockCutter
{
    uint64_t maxReads, maxLetters;
    uint64_t reads = 0, letters = 0; // of the open block

    explicit BlockCutter(uint64_t maxReads_, uint64_t maxLetters_ = kBlockLetters) : maxReads(maxReads_), maxLetters(maxLetters_) {}
    // a read of `n` letters joins the open block; true: the block is full and closes behind this read
    bool add(uint64_t n)
    {
        ++reads;
        letters += n;
        if (reads < maxReads && letters < maxLetters)
            return false;
        reads = letters = 0;
        return true;
    }
    bool open() const { return reads != 0; } // reads wait in a block that has not closed
};

// calls f(id, letters) per record of a FASTA or FASTQ text, until f returns false
template <class F>
void forEachRecord(std::string const & text, std::string const & path, F && f)
{
    RecordParser parser(path);
    if (parser.feed(text.data(), text.size(), f))
        parser.finish(f);
}

} // namespace lx_query_blocks
