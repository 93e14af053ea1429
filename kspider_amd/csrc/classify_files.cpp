// The file driver of classify: FASTA / FASTQ records in, two TSV files out.  Host only; the device part is the
// session of classify.hip (ksp_classify_open / _add / _finish), the host mode's ksp::ClassifyCpu (classify_cpu.cpp).
//   feed, batch  fastx_feed.h, shared with the sketch driver: every record is a source, a window is ksize bytes.  A record cut
//            across batches has every window in exactly one piece; the session counts a hash found in two pieces once.
//   pipeline two batch buffers (page-locked in device mode): the next one is filled by a thread while this one is hashed
//   write    both files at the end, each through .partial and a rename
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <iostream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/kspider_amd.h"
#include "engine_internal.h"
#include "fastx_feed.h"
#include "partial_file.h"
#include "sketch_set.h"

extern "C" int kspider_classify(const char* input, int kSize, uint64_t scaled, const char* db, const char* out_prefix, int user_threads, uint32_t min_hits) {
    const char* who = "kspider_classify";
    if (!input || !*input || !db || !*db || !out_prefix || !*out_prefix) { ksp::set_error(std::string(who) + ": input, db and out_prefix are required"); return KSP_E_ARG; }
    if (kSize < 1 || kSize > 64) { ksp::set_error(std::string(who) + ": kSize is 1 .. 64"); return KSP_E_ARG; }
    if (min_hits == 0) { ksp::set_error(std::string(who) + ": min_hits is 1 or more"); return KSP_E_ARG; }
    uint64_t max_hash = 0;
    if (const int rc = ksp_sketch_max_hash(scaled, &max_hash)) return rc;
    uint8_t* bufs[2] = {nullptr, nullptr};
    bool on_host = false;
    int rc = KSP_OK;
    ksp_classify* session = nullptr;
    ksp_classify_row* rows = nullptr;
    try {
        const char* how = std::getenv("KSPIDER_CLASSIFY");
        if (how && *how && std::strcmp(how, "host") != 0 && std::strcmp(how, "device") != 0) throw ArgError("KSPIDER_CLASSIFY is \"host\" or \"device\"");
        on_host = how && std::strcmp(how, "host") == 0;
        const int threads = user_threads < 1 ? 1 : user_threads;
        const uint32_t seed = 42u;
        const size_t batch_bytes = (size_t)env_bytes("KSPIDER_CLASSIFY_BATCH_BYTES", env_bytes("KSPIDER_CLASSIFY_BATCH_MB", 256, 1) << 20, 1024);
        const char* dv = std::getenv("KSPIDER_DEVICE");
        const int device = dv ? std::atoi(dv) : 0;
        // ---- the references: the groups of the database that have a sketch, in the database's order
        ksp::SketchSet set;
        if (is_directory(db)) {
            ksp::sketch_set_from_dir(db, kSize, threads, set);
        } else {
            ksp::read_sketch_pack(db, set);
            if (set.ksize != 0 && set.ksize != kSize)   // (0: packed from .bin files, whose k-mer size nobody wrote down)
                throw ArgError(std::string(db) + " was packed with kSize " + std::to_string(set.ksize) + ", not " + std::to_string(kSize));
        }
        std::vector<uint32_t> group_of;   // reference -> group (index into set.names)
        for (size_t g = 0; g < set.names.size(); ++g)
            if (set.present[g]) group_of.push_back((uint32_t)g);
        const uint32_t n_refs = (uint32_t)group_of.size();
        if (set.offsets.size() != (size_t)n_refs + 1) throw std::runtime_error(std::string(db) + ": the sketches and the groups that have one differ in number");
        ksp::ClassifyCpu cpu;
        if (on_host) {
            if ((rc = ksp::check_classify_refs(who, kSize, set.keys.data(), set.offsets.data(), n_refs))) throw CallError{rc};
            if ((rc = cpu.open(who, kSize, max_hash, seed, set.keys.data(), set.offsets.data(), n_refs))) throw CallError{rc};
        } else if ((rc = ksp_classify_open(device, kSize, max_hash, seed, set.keys.data(), set.offsets.data(), n_refs, &session))) {
            throw CallError{rc};
        }
        std::vector<uint64_t>().swap(set.keys);   // (the session has its table)
        Feed feed(input_files(input, kDnaEndings), FeedUnit::kRecord, threads, batch_bytes, kSize, kDnaEndings);
        for (uint8_t*& p : bufs) {
            p = (uint8_t*)(on_host ? std::malloc(batch_bytes) : ksp::pinned_alloc(batch_bytes));
            if (!p) throw std::bad_alloc();
        }
        Batch batch[2];
        batch[0].buf = bufs[0];
        batch[1].buf = bufs[1];
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
            const Batch& b = batch[cur];
            int run_rc = KSP_OK;
            if (!b.source.empty())
                run_rc = on_host ? cpu.add(who, b.buf, b.off.data(), b.source.data(), (uint32_t)b.source.size())
                                 : ksp_classify_add(session, b.buf, b.n_bytes, b.off.data(), b.source.data(), (uint32_t)b.source.size());
            filler.join();
            if (run_rc != KSP_OK) throw CallError{run_rc};
            if (fill_err) std::rethrow_exception(fill_err);
            more = more_next;
            cur ^= 1;
        }
        // ---- the results
        const size_t n_rec = feed.names.size();
        std::vector<uint32_t> kept(n_rec + 1), matched(n_rec + 1), refs(n_rec + 1), best_ref(n_rec + 1), best(n_rec + 1), second(n_rec + 1);
        uint64_t n_rows = 0;
        ksp_classify_stats st;
        std::memset(&st, 0, sizeof st);
        rc = on_host ? cpu.finish(who, (uint32_t)n_rec, min_hits, &rows, &n_rows, kept.data(), matched.data(), refs.data(), best_ref.data(), best.data(), second.data(), &st)
                     : ksp_classify_finish(session, (uint32_t)n_rec, min_hits, &rows, &n_rows, kept.data(), matched.data(), refs.data(), best_ref.data(), best.data(),
                                           second.data(), &st);
        if (rc != KSP_OK) throw CallError{rc};
        std::string summary = "record_id\tname\tlength\tkept_windows\tmatched\tn_refs\tbest_ref\tbest_hits\tsecond_hits\n";
        for (size_t r = 0; r < n_rec; ++r) {
            summary += std::to_string(r + 1) + '\t' + feed.names[r] + '\t' + std::to_string(feed.lengths[r]) + '\t' + std::to_string(kept[r]) + '\t' + std::to_string(matched[r]) +
                       '\t' + std::to_string(refs[r]) + '\t';
            if (best_ref[r] == 0xFFFFFFFFu) summary += '-';
            else if (best_ref[r] < n_refs) summary += set.names[group_of[best_ref[r]]];
            else throw std::runtime_error("a best reference that is none");
            summary += '\t' + std::to_string(best[r]) + '\t' + std::to_string(second[r]) + '\n';
        }
        std::string hits = "record_id\tname\tref_id\tref_name\thits\n";
        for (uint64_t i = 0; i < n_rows; ++i) {
            const ksp_classify_row& x = rows[i];
            if (x.record >= n_rec || x.reference >= n_refs) throw std::runtime_error("a row that names no record or no reference");
            hits += std::to_string(x.record + 1) + '\t' + feed.names[x.record] + '\t' + std::to_string(group_of[x.reference] + 1) + '\t' + set.names[group_of[x.reference]] + '\t' +
                    std::to_string(x.hits) + '\n';
        }
        ksp::write_file_atomically(std::string(out_prefix) + "_kSpider_classify.tsv", summary);
        ksp::write_file_atomically(std::string(out_prefix) + "_kSpider_classify_hits.tsv", hits);
        if (std::getenv("KSPIDER_VERBOSE"))
            std::cout << "kspider_amd: classify: " << n_rec << " records against " << n_refs << " references in " << st.batches << " batches" << (on_host ? " on the host" : "")
                      << "; " << st.bases << " bases, " << st.valid_kmers << " k-mers, " << st.kept_windows << " kept, " << st.hit_words << " hit words, "
                      << st.hit_words_unique << " distinct, " << st.table_keys << " table keys, " << st.rows << " rows; " << st.retries << " retries, " << st.compactions
                      << " compactions, " << st.workgroups << " workgroups; table " << st.ms_table << " ms, hash " << st.ms_hash << " ms, finish " << st.ms_finish << " ms"
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
    ksp_free(rows);
    if (session) ksp_classify_close(session);
    for (uint8_t* p : bufs) {
        if (on_host) std::free(p);
        else ksp::pinned_free(p);
    }
    return rc;
}
