// The sketches of a directory as the direct sketch inputs take them (sketch_loaders.cpp), and the pack file that keeps them
// (sketch_pack.cpp).  Host only.
#ifndef KSPIDER_SKETCH_SET_H
#define KSPIDER_SKETCH_SET_H
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace ksp {

struct SketchSource {
    uint32_t id = 0;
    uint32_t kmers = 0;           // what the reference stores in groupID_to_kmerCount
    std::vector<uint64_t> run;    // sorted unique hashes
    std::vector<uint32_t> abund;  // parallel to run when the signature has "abundances" (has_abund), else empty
    bool has_abund = false;
};
typedef std::vector<std::pair<uint32_t, std::string>> SketchNames;   // (group id, group name), ids 1, 2, ... in glob order

// Every .sig / .gz file of DIR as kspider_pairwise_sigs reads it: names = all groups; src = the groups that have a signature of
// that ksize, ascending by id.  Throws std::runtime_error (no such file, malformed JSON, no signature of that ksize).
void load_sig_dir(const std::string& dir, int kSize, int threads, SketchNames& names, std::vector<SketchSource>& src);
// Every .bin file of DIR as kspider_pairwise_bins reads it: every group has a source.
void load_bin_dir(const std::string& dir, int threads, SketchNames& names, std::vector<SketchSource>& src);

// One side of a query, from a directory or from a pack file: the names of all groups (group id = index + 1), per group whether
// it has a sketch and its k-mer count, and the runs of the groups that have one, in id order.
struct SketchSet {
    int ksize = 0;
    std::vector<std::string> names;
    std::vector<uint8_t> present;
    std::vector<uint32_t> kmers;      // per group; 0 without a sketch
    std::vector<uint64_t> offsets;    // present groups + 1
    std::vector<uint64_t> keys;
    // optional: filled from a directory of signatures only, and not kept by the pack file
    std::vector<uint8_t> counted;     // per group: its signature has abundances
    std::vector<uint32_t> abund;      // per key, parallel to keys (0 for a sketch without abundances); empty when no sketch has any
};
// mins and, when abunds is given, the abundance beside each, sorted by hash; a hash listed twice once, its abundances added and
// clamped at 2^32 - 1
void sort_sig_mins(std::vector<uint64_t>& mins, std::vector<uint32_t>* abunds);
// the directory's sketches (kSize > 0: load_sig_dir, kSize = 0: load_bin_dir) as a set
void sketch_set_from_dir(const std::string& dir, int kSize, int threads, SketchSet& out);
// The pack file format (little-endian, fixed width; every section padded to 8 bytes):
//   header   "KSPPACK1" | u32 version = 1 | i32 kSize | u64 groups G | u64 groups with a sketch S | u64 keys K | u64 name bytes B
//   kmers    G x u32        presence  G x u8        offsets  (S + 1) x u64
//   names    u64 count = G | (G + 1) x u64 offsets into the text | B bytes of text
//   keys     K x u64, the runs back to back, each strictly ascending
// write: through out_path.partial and a rename (partial_file.h); throws std::runtime_error.
void write_sketch_pack(const std::string& out_path, const SketchSet& set);
// read: `out` is written only when the whole file has been read and checked.  Throws std::runtime_error naming the first thing
// that is wrong: the magic or the version, a length that is not exactly what the header implies, a presence count or a name
// count that disagrees with the header, offsets that do not start at 0, decrease or end elsewhere, a run that is not strictly
// ascending.
void read_sketch_pack(const std::string& path, SketchSet& out);

}  // namespace ksp
#endif
