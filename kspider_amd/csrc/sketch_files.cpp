// The file driver of the sketcher: FASTA / FASTQ files in, one sourmash-compatible .sig file per source out.
// Host only; the device part is ksp_sketch_host (sketcher.hip), the host mode's ksp_sketch_cpu (sketch_cpu.cpp); with a molecule
// flag their _mol forms over protein files or DNA to translate, and a window of ksize residues or 3 ksize bases.
//   feed, batch  fastx_feed.h, shared with the classify driver: the window is ksize bytes, 3 ksize of translated input.  A source's
//            sketch is the union of its segments' sketches; with KSP_SKETCH_ABUND the counts of a hash in its segments are added
//            (every window lies in exactly one segment) and clamped after adding.
//   pipeline two batch buffers (page-locked in device mode): the next one is filled by a thread while this one is hashed
//   write    the signatures at the end, each through .partial and a rename
#include <glob.h>
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <exception>
#include <iostream>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/kspider_amd.h"
#include "engine_internal.h"
#include "fastx_feed.h"
#include "partial_file.h"

namespace {

// ---- MD5 (RFC 1321) of a text handed over in pieces ----
class Md5 {
    uint32_t a_ = 0x67452301u, b_ = 0xefcdab89u, c_ = 0x98badcfeu, d_ = 0x10325476u;
    uint64_t bytes_ = 0;
    unsigned char buf_[64];

    static uint32_t rotl(const uint32_t x, const int s) { return (x << s) | (x >> (32 - s)); }
    void block(const unsigned char* p) {
        static const uint32_t K[64] = {
            0xd76aa478, 0xe8c7b756, 0x242070db, 0xc1bdceee, 0xf57c0faf, 0x4787c62a, 0xa8304613, 0xfd469501, 0x698098d8, 0x8b44f7af, 0xffff5bb1,
            0x895cd7be, 0x6b901122, 0xfd987193, 0xa679438e, 0x49b40821, 0xf61e2562, 0xc040b340, 0x265e5a51, 0xe9b6c7aa, 0xd62f105d, 0x02441453,
            0xd8a1e681, 0xe7d3fbc8, 0x21e1cde6, 0xc33707d6, 0xf4d50d87, 0x455a14ed, 0xa9e3e905, 0xfcefa3f8, 0x676f02d9, 0x8d2a4c8a, 0xfffa3942,
            0x8771f681, 0x6d9d6122, 0xfde5380c, 0xa4beea44, 0x4bdecfa9, 0xf6bb4b60, 0xbebfbc70, 0x289b7ec6, 0xeaa127fa, 0xd4ef3085, 0x04881d05,
            0xd9d4d039, 0xe6db99e5, 0x1fa27cf8, 0xc4ac5665, 0xf4292244, 0x432aff97, 0xab9423a7, 0xfc93a039, 0x655b59c3, 0x8f0ccc92, 0xffeff47d,
            0x85845dd1, 0x6fa87e4f, 0xfe2ce6e0, 0xa3014314, 0x4e0811a1, 0xf7537e82, 0xbd3af235, 0x2ad7d2bb, 0xeb86d391};
        static const int S[64] = {7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 5, 9, 14, 20, 5, 9, 14, 20, 5, 9, 14, 20, 5, 9, 14, 20,
                                  4, 11, 16, 23, 4, 11, 16, 23, 4, 11, 16, 23, 4, 11, 16, 23, 6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21};
        uint32_t m[16];
        for (int i = 0; i < 16; ++i) m[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
        uint32_t a = a_, b = b_, c = c_, d = d_;
        for (int i = 0; i < 64; ++i) {
            uint32_t f;
            int g;
            if (i < 16) { f = (b & c) | (~b & d); g = i; }
            else if (i < 32) { f = (d & b) | (~d & c); g = (5 * i + 1) & 15; }
            else if (i < 48) { f = b ^ c ^ d; g = (3 * i + 5) & 15; }
            else { f = c ^ (b | ~d); g = (7 * i) & 15; }
            const uint32_t t = d;
            d = c;
            c = b;
            b = b + rotl(a + f + K[i] + m[g], S[i]);
            a = t;
        }
        a_ += a; b_ += b; c_ += c; d_ += d;
    }

public:
    void add(const char* p, size_t n) {
        while (n) {
            const size_t fill = (size_t)(bytes_ & 63), take = std::min<size_t>(n, 64 - fill);
            std::memcpy(buf_ + fill, p, take);
            bytes_ += take; p += take; n -= take;
            if (((bytes_) & 63) == 0) block(buf_);
        }
    }
    std::string hex() {
        const uint64_t bits = bytes_ * 8;
        const char one = (char)0x80, zero = 0;
        add(&one, 1);
        while ((bytes_ & 63) != 56) add(&zero, 1);
        unsigned char len[8];
        for (int i = 0; i < 8; ++i) len[i] = (unsigned char)(bits >> (8 * i));
        add((const char*)len, 8);
        static const char* digits = "0123456789abcdef";
        std::string out;
        for (const uint32_t w : {a_, b_, c_, d_})
            for (int i = 0; i < 4; ++i) {
                const unsigned byte = (w >> (8 * i)) & 0xFF;
                out += digits[byte >> 4];
                out += digits[byte & 15];
            }
        return out;
    }
};

// what kspider_sketch hashes: the molecule type, whether the bytes are DNA to translate, the bytes of a window, and what the
// signature says (sourmash stores ksize * 3 for the protein types)
struct Molecule {
    int type = KSP_MOL_DNA;
    bool translate = false;
    int window = 0, stored_ksize = 0;
    const char* name = "DNA";
    const std::vector<std::string>* endings = &kDnaEndings;
};

std::string json_text(const std::string& s) {
    std::string out = "\"";
    char buf[8];
    for (const unsigned char c : s) {
        if (c == '"' || c == '\\') { out += '\\'; out += (char)c; }
        else if (c < 0x20) { std::snprintf(buf, sizeof buf, "\\u%04x", c); out += buf; }
        else out += (char)c;
    }
    return out + "\"";
}

// the signature file of one source: the fields of the files sourmash writes, in a fixed order; abund: "abundances" behind "mins"
std::string sig_text(const std::string& filename, const int ksize, const char* molecule, const uint32_t seed, const uint64_t max_hash, const std::vector<uint64_t>& mins,
                     const std::vector<uint32_t>* abund) {
    std::string list;
    Md5 md5;
    char num[24];
    int n = std::snprintf(num, sizeof num, "%d", ksize);
    md5.add(num, (size_t)n);
    for (size_t i = 0; i < mins.size(); ++i) {
        n = std::snprintf(num, sizeof num, "%llu", (unsigned long long)mins[i]);
        md5.add(num, (size_t)n);
        if (i) list += ',';
        list.append(num, (size_t)n);
    }
    if (abund) {   // (the MD5 is over ksize and the mins alone, as sourmash's)
        list += "],\"abundances\":[";
        for (size_t i = 0; i < abund->size(); ++i) {
            if (i) list += ',';
            list += std::to_string((*abund)[i]);
        }
    }
    return "[{\"class\":\"sourmash_signature\",\"email\":\"\",\"hash_function\":\"0.murmur64\",\"filename\":" + json_text(filename) +
           ",\"license\":\"CC0\",\"version\":0.4,\"signatures\":[{\"num\":0,\"ksize\":" + std::to_string(ksize) + ",\"seed\":" + std::to_string(seed) +
           ",\"max_hash\":" + std::to_string(max_hash) + ",\"molecule\":\"" + molecule + "\",\"md5sum\":\"" + md5.hex() + "\",\"mins\":[" + list + "]}]}]\n";
}

// the sketches of one batch, appended to the keys of their sources (counts: and their counts to `counts`)
void run_batch(const Batch& b, const bool on_host, const int device, const int ksize, const Molecule& mol, const uint64_t max_hash, const uint32_t seed,
               std::vector<std::vector<uint64_t>>& keys, std::vector<std::vector<uint32_t>>* counts, std::vector<uint32_t>& segments, ksp_sketch_stats& total) {
    const uint32_t n_seg = (uint32_t)b.source.size();
    if (n_seg == 0) return;
    std::vector<uint64_t> out_off((size_t)n_seg + 1, 0), host_keys;
    std::vector<uint32_t> host_abund;
    uint64_t* got = nullptr;
    uint32_t* got_abund = nullptr;
    const uint64_t mol_flags = mol.translate ? KSP_SKETCH_TRANSLATE : 0;
    if (on_host) {
        uint64_t needed = 0;
        const double share = ((double)max_hash + 1.0) / 18446744073709551616.0;
        host_keys.resize((size_t)std::min<uint64_t>(b.n_bytes, (uint64_t)((double)b.n_bytes * share * 1.25) + 4096));
        const auto call = [&]() {
            if (mol.type != KSP_MOL_DNA) {
                if (counts) host_abund.resize(host_keys.size() + 1);   // (+ 1: not NULL with room for nothing, which would ask for the plain sketch)
                return ksp_sketch_cpu_mol(b.buf, b.n_bytes, b.off.data(), n_seg, ksize, mol.type, mol_flags, max_hash, seed, host_keys.data(), counts ? host_abund.data() : nullptr,
                                          host_keys.size(), out_off.data(), &needed);
            }
            if (!counts) return ksp_sketch_cpu(b.buf, b.n_bytes, b.off.data(), n_seg, ksize, max_hash, seed, host_keys.data(), host_keys.size(), out_off.data(), &needed);
            host_abund.resize(host_keys.size());
            return ksp_sketch_cpu_abund(b.buf, b.n_bytes, b.off.data(), n_seg, ksize, max_hash, seed, host_keys.data(), host_abund.data(), host_keys.size(), out_off.data(), &needed);
        };
        int rc = call();
        if (rc == KSP_E_OVERFLOW) {
            host_keys.resize((size_t)needed);
            rc = call();
        }
        if (rc != KSP_OK) throw CallError{rc};
        got = host_keys.data();
        got_abund = host_abund.data();
    } else {
        ksp_sketch_stats st;
        const int rc = mol.type != KSP_MOL_DNA
                           ? ksp_sketch_host_mol(device, b.buf, b.n_bytes, b.off.data(), n_seg, ksize, mol.type, mol_flags, max_hash, seed, &got, counts ? &got_abund : nullptr, out_off.data(), &st)
                       : counts ? ksp_sketch_host_abund(device, b.buf, b.n_bytes, b.off.data(), n_seg, ksize, max_hash, seed, &got, &got_abund, out_off.data(), &st)
                              : ksp_sketch_host(device, b.buf, b.n_bytes, b.off.data(), n_seg, ksize, max_hash, seed, &got, out_off.data(), &st);
        if (rc != KSP_OK) throw CallError{rc};
        total.bases += st.bases; total.valid_kmers += st.valid_kmers; total.kept += st.kept; total.distinct_out += st.distinct_out;
        total.retries += st.retries; total.ms_upload += st.ms_upload; total.ms_hash += st.ms_hash; total.ms_select += st.ms_select;
    }
    for (uint32_t s = 0; s < n_seg; ++s) {
        const uint32_t src = b.source[s];
        if (src >= keys.size()) { keys.resize((size_t)src + 1); segments.resize((size_t)src + 1, 0); }
        keys[src].insert(keys[src].end(), got + out_off[s], got + out_off[s + 1]);
        if (counts) {
            if (src >= counts->size()) counts->resize((size_t)src + 1);
            (*counts)[src].insert((*counts)[src].end(), got_abund + out_off[s], got_abund + out_off[s + 1]);
        }
        ++segments[src];
    }
    if (!on_host) { ksp_free(got); ksp_free(got_abund); }
}

}  // namespace

extern "C" int kspider_sketch(const char* input, int kSize, uint64_t scaled, const char* out_dir, int user_threads, uint64_t flags) {
    const char* who = "kspider_sketch";
    if (!input || !*input || !out_dir || !*out_dir) { ksp::set_error(std::string(who) + ": input and out_dir are required"); return KSP_E_ARG; }
    if (kSize < 1 || kSize > 64) { ksp::set_error(std::string(who) + ": kSize is 1 .. 64"); return KSP_E_ARG; }
    Molecule mol;
    {
        const uint64_t types = flags & (KSP_SKETCH_PROTEIN | KSP_SKETCH_DAYHOFF | KSP_SKETCH_HP);
        if (types & (types - 1)) { ksp::set_error(std::string(who) + ": KSP_SKETCH_PROTEIN, _DAYHOFF and _HP exclude each other"); return KSP_E_ARG; }
        mol.translate = (flags & KSP_SKETCH_TRANSLATE) != 0;
        if (mol.translate && !types) { ksp::set_error(std::string(who) + ": KSP_SKETCH_TRANSLATE needs KSP_SKETCH_PROTEIN, _DAYHOFF or _HP"); return KSP_E_ARG; }
        if (mol.translate && kSize > 21) { ksp::set_error(std::string(who) + ": kSize is 1 .. 21 with KSP_SKETCH_TRANSLATE (3 * kSize <= 63 bases)"); return KSP_E_ARG; }
        if (types) {
            mol.type = types == KSP_SKETCH_PROTEIN ? KSP_MOL_PROTEIN : types == KSP_SKETCH_DAYHOFF ? KSP_MOL_DAYHOFF : KSP_MOL_HP;
            mol.name = types == KSP_SKETCH_PROTEIN ? "protein" : types == KSP_SKETCH_DAYHOFF ? "dayhoff" : "hp";
            if (!mol.translate) mol.endings = &kProteinEndings;
        }
        mol.window = mol.translate ? 3 * kSize : kSize;
        mol.stored_ksize = types ? 3 * kSize : kSize;
    }
    uint64_t max_hash = 0;
    if (const int rc = ksp_sketch_max_hash(scaled, &max_hash)) return rc;
    uint8_t* bufs[2] = {nullptr, nullptr};
    bool on_host = false;
    int rc = KSP_OK;
    try {
        const char* how = std::getenv("KSPIDER_SKETCH");
        if (how && *how && std::strcmp(how, "host") != 0 && std::strcmp(how, "device") != 0) throw ArgError("KSPIDER_SKETCH is \"host\" or \"device\"");
        on_host = how && std::strcmp(how, "host") == 0;
        const int threads = user_threads < 1 ? 1 : user_threads;
        const uint32_t seed = (flags & KSP_SKETCH_SEED) ? (uint32_t)(flags >> 32) : 42u;
        const bool per_record = (flags & KSP_SKETCH_PER_RECORD) != 0, counted = (flags & KSP_SKETCH_ABUND) != 0;
        if (per_record && is_directory(input)) throw ArgError("KSP_SKETCH_PER_RECORD takes one file, not a directory");
        const size_t batch_bytes = (size_t)env_bytes("KSPIDER_SKETCH_BATCH_BYTES", env_bytes("KSPIDER_SKETCH_BATCH_MB", 256, 1) << 20, 1024);
        const char* dv = std::getenv("KSPIDER_DEVICE");
        const int device = dv ? std::atoi(dv) : 0;
        Feed feed(input_files(input, *mol.endings), per_record ? FeedUnit::kRecordAsFile : FeedUnit::kFile, threads, batch_bytes, mol.window, *mol.endings);
        for (uint8_t*& p : bufs) {
            p = (uint8_t*)(on_host ? std::malloc(batch_bytes) : ksp::pinned_alloc(batch_bytes));
            if (!p) throw std::bad_alloc();
        }
        Batch batch[2];
        batch[0].buf = bufs[0];
        batch[1].buf = bufs[1];
        std::vector<std::vector<uint64_t>> keys;
        std::vector<std::vector<uint32_t>> counts;
        std::vector<uint32_t> segments;
        ksp_sketch_stats total;
        std::memset(&total, 0, sizeof total);
        uint64_t n_batches = 0;
        // ---- the pipeline: batch `cur` is hashed while a thread fills the other
        int cur = 0;
        bool more = feed.fill(batch[cur]);
        while (more) {
            bool more_next = false;
            std::exception_ptr fill_err;
            std::thread filler([&]() {
                try {
                    more_next = feed.fill(batch[cur ^ 1]);
                } catch (...) {
                    fill_err = std::current_exception();
                }
            });
            std::exception_ptr run_err;
            try {
                run_batch(batch[cur], on_host, device, kSize, mol, max_hash, seed, keys, counted ? &counts : nullptr, segments, total);
                ++n_batches;
            } catch (...) {
                run_err = std::current_exception();
            }
            filler.join();
            if (run_err) std::rethrow_exception(run_err);
            if (fill_err) std::rethrow_exception(fill_err);
            more = more_next;
            cur ^= 1;
        }
        // ---- the sources: names, unions, files
        const size_t n_src = feed.names.size();
        keys.resize(n_src);
        counts.resize(n_src);
        segments.resize(n_src, 0);
        {
            std::set<std::string> seen;
            for (const std::string& n : feed.names) {
                if (n.empty()) throw ArgError("a source without a name");
                if (!seen.insert(n).second) throw ArgError("two sources are named " + n);
            }
        }
        if (mkdir(out_dir, 0777) != 0 && errno != EEXIST) throw std::runtime_error(std::string("cannot create ") + out_dir);
        parallel_for(n_src, threads, [&](const size_t s) {
            std::vector<uint64_t>& k = keys[s];
            std::vector<uint32_t>& c = counts[s];
            if (segments[s] > 1 && counted) {   // the union with the counts added: a plain union would lose them
                std::vector<std::pair<uint64_t, uint32_t>> both(k.size());
                for (size_t i = 0; i < k.size(); ++i) both[i] = {k[i], c[i]};
                std::sort(both.begin(), both.end());
                k.clear();
                c.clear();
                for (size_t i = 0, j = 0; i < both.size(); i = j) {
                    uint64_t sum = 0;
                    for (; j < both.size() && both[j].first == both[i].first; ++j) sum = std::min<uint64_t>(sum + both[j].second, 0xFFFFFFFFull);
                    k.push_back(both[i].first);
                    c.push_back((uint32_t)sum);
                }
            } else if (segments[s] > 1) {
                std::sort(k.begin(), k.end());
                k.erase(std::unique(k.begin(), k.end()), k.end());
            }
            ksp::write_file_atomically(std::string(out_dir) + "/" + feed.names[s] + ".sig", sig_text(feed.filenames[s], mol.stored_ksize, mol.name, seed, max_hash, k, counted ? &c : nullptr));
        });
        if (std::getenv("KSPIDER_VERBOSE"))
            std::cout << "kspider_amd: sketch: " << n_src << " sources in " << n_batches << " batches" << (on_host ? " on the host" : "") << "; " << total.bases
                      << " bases, " << total.kept << " kept; upload " << total.ms_upload << " ms, hash " << total.ms_hash << " ms, select " << total.ms_select << " ms"
                      << std::endl;
    } catch (const CallError& e) {
        rc = e.rc;
    } catch (const std::bad_alloc&) {
        ksp::set_error(std::string(who) + ": out of host memory");
        rc = KSP_E_LIMIT;
    } catch (const ArgError& e) {
        ksp::set_error(std::string(who) + ": " + e.what());
        rc = KSP_E_ARG;
    } catch (const std::exception& e) {
        ksp::set_error(std::string(who) + ": " + e.what());
        rc = KSP_E_IO;
    }
    for (uint8_t* p : bufs) {
        if (on_host) std::free(p);
        else ksp::pinned_free(p);
    }
    return rc;
}
