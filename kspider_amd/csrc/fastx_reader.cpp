// The FASTA / FASTQ reader of the sketcher.  Host only.  A file, plain or gzip, is read whole; the first byte that
// is not white space says which of the two it is.  FASTA: a line starting with '>' opens a record, every other line is appended
// to the open record's bases.  FASTQ: records of exactly four lines — '@' header, bases, '+' line, qualities of the same length —,
// so a quality line may start with '@' or '>'.  Both: a trailing '\r' is dropped from every line, a final line without a newline
// counts, an empty record stays (its bases are no bytes).  The bases stand as they are in the file: case and break bytes are the
// hasher's business.
#include <cstdint>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/kspider_amd.h"
#include "engine_internal.h"

namespace {

// the lines of a text, one after the other, without their "\n" or "\r\n"
struct Lines {
    const std::string& text;
    size_t at = 0;
    uint64_t number = 0;   // of the line next() returned last, from 1
    bool next(const char** p, size_t* n) {
        if (at >= text.size()) return false;
        const char* s = text.data() + at;
        const char* e = (const char*)std::memchr(s, '\n', text.size() - at);
        size_t len = e ? (size_t)(e - s) : text.size() - at;
        at += len + (e ? 1 : 0);
        if (len && s[len - 1] == '\r') --len;
        ++number;
        *p = s;
        *n = len;
        return true;
    }
};

bool blank(const char* p, const size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (p[i] != ' ' && p[i] != '\t' && p[i] != '\r') return false;
    return true;
}

// the first word of a header line behind its '>' or '@'
std::string first_word(const char* p, const size_t n) {
    size_t a = 1;
    while (a < n && (p[a] == ' ' || p[a] == '\t')) ++a;
    size_t b = a;
    while (b < n && p[b] != ' ' && p[b] != '\t') ++b;
    return std::string(p + a, b - a);
}

template <class Fn>
int guarded(const char* who, Fn fn) {
    try {
        return fn();
    } catch (const std::bad_alloc&) {
        ksp::set_error(std::string(who) + ": out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(std::string(who) + ": " + e.what());
        return KSP_E_IO;
    }
}

}  // namespace

void ksp::read_fastx(const std::string& path, FastxFile& out) {
    const std::string text = read_maybe_gz(path);
    FastxFile f;
    f.rec_off.push_back(0);
    Lines in{text};
    const auto bad = [&](const std::string& what) { return std::runtime_error(path + ": line " + std::to_string(in.number) + ": " + what); };
    const char* p = nullptr;
    size_t n = 0;
    bool have = in.next(&p, &n);
    while (have && blank(p, n)) have = in.next(&p, &n);
    if (!have) { out = std::move(f); return; }   // an empty file has no record
    if (p[0] != '>' && p[0] != '@') throw bad("neither a FASTA ('>') nor a FASTQ ('@') header");
    f.fastq = p[0] == '@';
    f.seq.reserve(text.size());
    if (!f.fastq) {
        bool open = false;
        for (; have; have = in.next(&p, &n)) {
            if (n && p[0] == '>') {
                if (open) { f.seq.push_back('\n'); f.rec_off.push_back(f.seq.size()); }
                f.names.push_back(first_word(p, n));
                open = true;
            } else {
                f.seq.append(p, n);
            }
        }
        f.seq.push_back('\n');
        f.rec_off.push_back(f.seq.size());
    } else {
        while (have) {
            if (blank(p, n)) { have = in.next(&p, &n); continue; }   // (blank lines between records and at the end)
            if (p[0] != '@') throw bad("a FASTQ record starts with '@'");
            f.names.push_back(first_word(p, n));
            const char* b = nullptr;
            size_t nb = 0, nq = 0;
            if (!in.next(&b, &nb)) throw bad("the file ends inside a FASTQ record (no bases line)");
            if (!in.next(&p, &n)) throw bad("the file ends inside a FASTQ record (no '+' line)");
            if (n == 0 || p[0] != '+') throw bad("the third line of a FASTQ record starts with '+'");
            if (!in.next(&p, &nq)) {   // (an empty record at the end of a file without a final newline: its empty quality line is no line)
                if (nb != 0) throw bad("the file ends inside a FASTQ record (no quality line)");
                nq = 0;
            }
            if (nq != nb) throw bad("the quality line has " + std::to_string(nq) + " bytes, the bases " + std::to_string(nb));
            f.seq.append(b, nb);
            f.seq.push_back('\n');
            f.rec_off.push_back(f.seq.size());
            have = in.next(&p, &n);
        }
    }
    out = std::move(f);
}

extern "C" int ksp_fastx_info(const char* path, uint64_t out[4]) {
    const char* who = "ksp_fastx_info";
    if (!path || !out) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    return guarded(who, [&]() {
        ksp::FastxFile f;
        ksp::read_fastx(path, f);
        uint64_t text = 0;
        for (const std::string& s : f.names) text += s.size();
        out[0] = f.names.size();
        out[1] = f.seq.size();
        out[2] = text;
        out[3] = f.fastq ? 1 : 0;
        return (int)KSP_OK;
    });
}

extern "C" int ksp_fastx_load(const char* path, uint8_t* seq, uint64_t* rec_offsets, uint64_t* name_offsets, char* names) {
    const char* who = "ksp_fastx_load";
    if (!path || !seq || !rec_offsets || !name_offsets || !names) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    return guarded(who, [&]() {
        ksp::FastxFile f;
        ksp::read_fastx(path, f);
        if (!f.seq.empty()) std::memcpy(seq, f.seq.data(), f.seq.size());
        std::memcpy(rec_offsets, f.rec_off.data(), 8 * f.rec_off.size());
        uint64_t at = 0;
        for (size_t r = 0; r < f.names.size(); ++r) {
            name_offsets[r] = at;
            std::memcpy(names + at, f.names[r].data(), f.names[r].size());
            at += f.names[r].size();
        }
        name_offsets[f.names.size()] = at;
        return (int)KSP_OK;
    });
}
