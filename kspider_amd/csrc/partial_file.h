// Output files that appear under their final name complete or not at all: everything is written to PATH.partial and renamed
// at the end.  Host only, standard library only: the writers of the .hip files and of the g++-built sources both use it.
#ifndef KSPIDER_PARTIAL_FILE_H
#define KSPIDER_PARTIAL_FILE_H
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace ksp {

// The outputs of one call.  open() as many as the call writes, write to the streams, commit() once: all files are renamed to
// their final names.  Unless committed — an exception on the way, a failed write, a failed rename — the destructor removes
// every PATH.partial.  The streams are the caller's and have to live until commit().
class PartialFiles {
    std::vector<std::string> paths_;
    std::vector<std::ofstream*> streams_;
    bool committed_ = false;

    static std::string partial(const std::string& path) { return path + ".partial"; }

public:
    PartialFiles() = default;
    PartialFiles(const PartialFiles&) = delete;
    PartialFiles& operator=(const PartialFiles&) = delete;
    void open(const std::string& path, std::ofstream& f) {
        paths_.push_back(path);   // (listed first: a file that exists is one the destructor knows)
        streams_.push_back(&f);
        f.open(partial(path), std::ios::binary | std::ios::trunc);
        if (!f) {
            paths_.pop_back();
            streams_.pop_back();
            throw std::runtime_error("cannot write " + partial(path));
        }
    }
    void commit() {
        for (size_t i = 0; i < paths_.size(); ++i) {
            streams_[i]->flush();
            if (!*streams_[i]) throw std::runtime_error("write error on " + partial(paths_[i]));
            streams_[i]->close();
        }
        for (const std::string& p : paths_)
            if (std::rename(partial(p).c_str(), p.c_str()) != 0) throw std::runtime_error("cannot rename " + partial(p));
        committed_ = true;
    }
    ~PartialFiles() {
        if (committed_) return;
        for (const std::string& p : paths_) std::remove(partial(p).c_str());
    }
};

// `text` as the whole content of `path`
inline void write_file_atomically(const std::string& path, const std::string& text) {
    std::ofstream f;
    PartialFiles files;
    files.open(path, f);
    f.write(text.data(), (std::streamsize)text.size());
    files.commit();
}

}  // namespace ksp
#endif
