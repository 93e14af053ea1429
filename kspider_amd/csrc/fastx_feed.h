// What the file drivers over FASTA / FASTQ input share (sketch_files.cpp; classify_files.cpp): the
// input files of a path, the feed that reads them `threads` at a time and hands their bytes on as batches of segments, the
// errors a guarded entry throws, and the batch-size variables.  Host only; every name here has internal linkage.
//   feed     the input files in order, read `threads` at a time (fastx_reader.cpp); what is read and not yet sent waits as pieces
//   batch    at most `batch_bytes` bytes of pieces back to back, each a segment of one source.  A piece that does not fit is cut:
//            the batch takes what it has room for, and the rest starts window - 1 bytes before the cut, so every window lies
//            whole in exactly one of the two.
#ifndef KSPIDER_FASTX_FEED_H
#define KSPIDER_FASTX_FEED_H
#include <glob.h>
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <exception>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "engine_internal.h"

namespace {

// what a guarded entry throws for a bad argument (KSP_E_ARG instead of KSP_E_IO)
struct ArgError : std::runtime_error {
    using std::runtime_error::runtime_error;
};
// a compute call failed: its code, the text is already in ksp_last_error()
struct CallError {
    int rc;
};

bool is_directory(const std::string& path) {
    struct stat st;
    return stat(path.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}
std::string base_name(const std::string& path) { return path.substr(path.find_last_of("/\\") + 1); }
bool ends_with(const std::string& s, const std::string& e) { return s.size() >= e.size() && s.compare(s.size() - e.size(), e.size(), e) == 0; }

// the endings of the input files: nucleotide (DNA, and translated input), and protein
const std::vector<std::string> kDnaEndings{".fa", ".fasta", ".fna", ".fq", ".fastq"}, kProteinEndings{".faa", ".fa", ".fasta"};

// the file name without .gz and without its ending; "" when it has none of the endings
std::string source_name_of(const std::string& path, const std::vector<std::string>& endings) {
    std::string n = base_name(path);
    if (ends_with(n, ".gz")) n.resize(n.size() - 3);
    for (const std::string& e : endings)
        if (ends_with(n, e) && n.size() > e.size()) return n.substr(0, n.size() - e.size());
    return "";
}

// fn(i) for i in [0, n) on up to `threads` host threads; the first exception is rethrown on the caller
template <class Fn>
void parallel_for(const size_t n, const int threads, Fn fn) {
    const size_t nt = std::max<size_t>(1, std::min<size_t>({(size_t)std::max(1, threads), n, 64}));
    if (nt <= 1) { for (size_t i = 0; i < n; ++i) fn(i); return; }
    std::atomic<size_t> next{0};
    std::exception_ptr err;
    std::mutex mu;
    std::vector<std::thread> th;
    for (size_t t = 0; t < nt; ++t)
        th.emplace_back([&]() {
            try {
                for (size_t i = next.fetch_add(1); i < n; i = next.fetch_add(1)) fn(i);
            } catch (...) {
                std::lock_guard<std::mutex> g(mu);
                if (!err) err = std::current_exception();
            }
        });
    for (auto& t : th) t.join();
    if (err) std::rethrow_exception(err);
}

// bytes of one source that are read and not yet in a batch
struct Piece {
    uint32_t source;
    std::shared_ptr<const std::string> text;
    size_t at, end;
};

// one batch: segments of sources back to back
struct Batch {
    uint8_t* buf = nullptr;
    size_t n_bytes = 0;
    std::vector<uint64_t> off{0};    // the segments' bounds
    std::vector<uint32_t> source;    // the source of every segment
    void clear() { n_bytes = 0; off.assign(1, 0); source.clear(); }
};

// what a source is: a file; a record, named for a file of its own (a '/' of the name becomes '_'); or a record as it is named,
// with the bytes of its sequence in `lengths`
enum class FeedUnit { kFile, kRecordAsFile, kRecord };

// The input in order.  Only one thread at a time calls fill().
class Feed {
    std::vector<std::string> files_;
    size_t next_file_ = 0;
    FeedUnit unit_;
    int threads_;
    size_t batch_bytes_, overlap_;
    const std::vector<std::string>& endings_;
    std::deque<Piece> pieces_;

    void read_more() {
        const size_t n = std::min<size_t>((size_t)std::max(1, threads_), files_.size() - next_file_);
        std::vector<ksp::FastxFile> read(n);
        parallel_for(n, threads_, [&](const size_t i) { ksp::read_fastx(files_[next_file_ + i], read[i]); });
        for (size_t i = 0; i < n; ++i) {
            const std::string& path = files_[next_file_ + i];
            ksp::FastxFile& f = read[i];
            const size_t n_rec = f.names.size();
            const auto text = std::make_shared<const std::string>(std::move(f.seq));
            if (unit_ != FeedUnit::kFile) {
                for (size_t r = 0; r < n_rec; ++r) {
                    std::string name = f.names[r];
                    if (unit_ == FeedUnit::kRecordAsFile) {
                        std::replace(name.begin(), name.end(), '/', '_');
                        filenames.push_back(base_name(path));
                    } else {
                        lengths.push_back(f.rec_off[r + 1] - f.rec_off[r] - 1);   // (without the newline the reader puts behind a record)
                    }
                    names.push_back(name);
                    pieces_.push_back(Piece{(uint32_t)(names.size() - 1), text, (size_t)f.rec_off[r], (size_t)f.rec_off[r + 1]});
                }
            } else {
                const std::string by_ending = source_name_of(path, endings_);
                names.push_back(by_ending.empty() ? base_name(path) : by_ending);
                filenames.push_back(base_name(path));
                pieces_.push_back(Piece{(uint32_t)(names.size() - 1), text, 0, text->size()});
            }
            if (names.size() > 0xFFFFFFFEull) throw std::runtime_error("more than 2^32 - 2 sources");
        }
        next_file_ += n;
    }

public:
    std::vector<std::string> names, filenames;   // of every source met so far (read by the caller only after the last fill())
    std::vector<uint64_t> lengths;               // FeedUnit::kRecord: the bytes of every record's sequence

    // window: the bytes of one window (ksize; 3 * ksize of translated input)
    Feed(std::vector<std::string> files, const FeedUnit unit, const int threads, const size_t batch_bytes, const int window, const std::vector<std::string>& endings)
        : files_(std::move(files)), unit_(unit), threads_(threads), batch_bytes_(batch_bytes), overlap_((size_t)window - 1), endings_(endings) {}

    // the next batch; false when the input is used up and the batch is empty
    bool fill(Batch& b) {
        b.clear();
        for (;;) {
            if (pieces_.empty()) {
                if (next_file_ >= files_.size()) break;
                read_more();
                continue;
            }
            Piece& p = pieces_.front();
            const size_t left = p.end - p.at, room = batch_bytes_ - b.n_bytes;
            if (left == 0) { pieces_.pop_front(); continue; }
            if (left > room && room <= 2 * overlap_ + 16) break;   // too little room to cut into: the batch is full
            const size_t take = std::min(left, room);
            std::memcpy(b.buf + b.n_bytes, p.text->data() + p.at, take);
            b.n_bytes += take;
            b.off.push_back(b.n_bytes);
            b.source.push_back(p.source);
            if (take == left) { pieces_.pop_front(); continue; }
            p.at += take - overlap_;   // the rest starts window - 1 bytes before the cut
            break;
        }
        return b.n_bytes > 0 || !pieces_.empty() || next_file_ < files_.size();
    }
};

std::vector<std::string> input_files(const std::string& input, const std::vector<std::string>& endings) {
    if (!is_directory(input)) return {input};
    std::string dir = input;
    while (dir.size() > 1 && dir.back() == '/') dir.pop_back();
    glob_t g;
    std::memset(&g, 0, sizeof g);
    const std::string pat = dir + "/*";
    const int rv = glob(pat.c_str(), GLOB_TILDE, nullptr, &g);   // the order of the sig loader
    std::vector<std::string> out;
    if (rv == 0)
        for (size_t i = 0; i < g.gl_pathc; ++i)
            if (!source_name_of(g.gl_pathv[i], endings).empty() && !is_directory(g.gl_pathv[i])) out.emplace_back(g.gl_pathv[i]);
    globfree(&g);
    if (rv != 0 && rv != GLOB_NOMATCH) throw std::runtime_error("glob() failed on " + pat);
    if (out.empty()) {
        std::string list;
        for (const std::string& e : endings) list += (list.empty() ? "" : " / ") + e;
        throw std::runtime_error("no " + list + " file (plain or .gz) in " + dir);
    }
    return out;
}

// $name as a number of at least `lo`, `fallback` when unset or empty
uint64_t env_bytes(const char* name, const uint64_t fallback, const uint64_t lo) {
    const char* s = std::getenv(name);
    if (!s || !*s) return fallback;
    char* end = nullptr;
    const unsigned long long v = std::strtoull(s, &end, 10);
    if (end == s || *end || *s == '-' || v < lo) throw ArgError(std::string(name) + " is a number of at least " + std::to_string(lo));
    return v;
}

}  // namespace
#endif
