// The hash passes of the sketcher; included into sketcher.hip's anonymous namespace.  One frame, sketch_tiles,
// holds what every pass does: a workgroup of 256 loops over tiles of kTile positions; per tile every thread loads 16 bytes (the
// first four another 16: the halo of 64 bytes; bytes behind the stream's end are breaks) and stages them with 16 break bits in
// LDS; then a thread takes the positions tid, tid + 256, ...: a window without a break bit is hashed; a hash <= max_hash finds
// its source by binary search of the offsets, is dropped when its window would cross the source's end, and is appended as
// (hash, source) with one returning add per wave; the counters are flushed at the end.  A kernel adds how a piece is staged and
// how a position is hashed:
//   k_sketch_hash<kWide>      DNA: a piece becomes 32 bits of 2-bit codes; the forward k-mer, left-aligned, is a funnel shift of two
//                             (kWide, k > 32: three) code words — no lane rolls over the bases before it; canonical form, text, Murmur.
//   k_sketch_hash_protein     the bytes are residues.  The tile sits in LDS as the letters that are hashed, one byte per position
//                             (0 for a break).  A lane reads the 32-bit words its k letters lie in — neighbouring lanes read
//                             neighbouring or the same words: no bank is asked for two addresses — and funnel-shifts them down
//                             by its byte offset, masks the tail, hashes.
//   k_sketch_hash_translated  the bytes are DNA, staged as in k_sketch_hash; the window is 3k bases.  The forward k-mer and its
//                             reverse complement are each translated codon by codon through a 64-byte LDS table and hashed: two
//                             possible survivors per position, appended together.
// The arithmetic is sketch_hash.h and sketch_mol.h, shared with the host loop.

constexpr int kThreads = 256;
constexpr u32 kTile = KSP_SKETCH_TILE_BASES;
constexpr u32 kChunks = kTile / 16 + 4;   // 16-byte pieces of a tile and its halo of 64 bytes
constexpr u32 kCodeWords = kChunks / 2;   // 32 bases per word
constexpr u32 kMaskWords = kChunks / 4;   // 64 positions per word
constexpr u32 kLetterWords = (kTile + 64) / 4;   // the tile's and the halo's letters as 32-bit words
static_assert(kTile == 16 * kThreads, "a thread loads one 16-byte piece of the tile");
static_assert(kTile % 64 == 0 && kChunks % 4 == 0, "whole mask words");

// a survivor: its hash and its source
struct Rec {
    u64 hash, src;
};

struct HashArgs {
    const uint8_t* seq;
    u64 n_bytes, n_tiles;
    const u64* src_off;   // n_sources + 1, device
    u32 n_sources, k, seed;   // k: bases, or for a molecule type residues, per k-mer
    u64 max_hash;
    Rec* recs;
    u64 capacity;
    unsigned long long* counters;   // [0] survivors, the ones without room included, [1] bases, [2] windows without a break
};

struct MolArgs {
    HashArgs h;
    int mol;   // KSP_MOL_PROTEIN / _DAYHOFF / _HP
};

// the sum of v over the wave, in lane 0
__device__ inline u32 wave_sum(u32 v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (u32)__shfl_down((int)v, d);
    return v;
}

// 16 bytes of the stream at `at` as four words; bytes at and behind n_bytes are 0, a break
__device__ __forceinline__ void load_piece(const uint8_t* seq, const u64 n_bytes, const u64 at, u32 w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    if (at + 16 <= n_bytes) {
        const uint4 v = *reinterpret_cast<const uint4*>(seq + at);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else if (at < n_bytes) {
        const u32 n = (u32)(n_bytes - at);   // 1 .. 15 bytes are left
#pragma unroll
        for (u32 j = 0; j < 16; ++j)
            if (j < n) w[j >> 2] |= (u32)seq[at + j] << (8 * (j & 3));
    }
}

// piece c of DNA bytes: its 32 bits of 2-bit codes into s_code (big-endian: base 32j of the tile on top of word j); returns its 16 break bits
__device__ __forceinline__ u32 stage_bases(const u32 w[4], const u32 c, u64* s_code) {
    u32 code = 0, breaks = 0;
#pragma unroll
    for (u32 j = 0; j < 16; ++j) {
        const u32 b = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        code |= sk::base_code(b) << (30 - 2 * j);
        breaks |= (sk::is_base(b) ? 0u : 1u) << j;
    }
    reinterpret_cast<u32*>(s_code)[c ^ 1u] = code;   // (the even piece is the upper half of its word)
    return breaks;
}

// whether none of the `win` (1 .. 64) positions from tile position p on is a break; s_mask is little-endian: bit i of word m =
// position 64m + i is a break
__device__ __forceinline__ bool window_unbroken(const u64* s_mask, const u32 p, const u32 win) {
    const u32 m = p >> 6, s = p & 63;
    const u64 window = s ? (s_mask[m] >> s) | (s_mask[m + 1] << (64 - s)) : s_mask[m];   // (m + 1 <= 64: the halo's word)
    return (window & (win == 64 ? ~0ull : (1ull << win) - 1)) == 0;
}

// the forward k-mer of the `win` bases from tile position p on, left-aligned, out of s_code; kWide: win > 32, the k-mer takes two words
template <bool kWide>
__device__ __forceinline__ sk::Kmer kmer_at(const u64* s_code, const u32 p, const u32 win) {
    const u32 j = p >> 5, s2 = 2 * (p & 31);
    sk::Kmer fw;
    fw.hi = s2 ? (s_code[j] << s2) | (s_code[j + 1] >> (64 - s2)) : s_code[j];
    fw.lo = 0;
    if (kWide) fw.lo = s2 ? (s_code[j + 1] << s2) | (s_code[j + 2] >> (64 - s2)) : s_code[j + 1];   // (j + 2 <= 129)
    return sk::keep_top(fw, win);
}

// the source of stream position gp (the last s with src_off[s] <= gp), and whether a window of `win` bytes at gp ends inside it:
// two sources may abut without a break byte, and a window over the end of its source is none
__device__ __forceinline__ bool window_in_source(const HashArgs& A, const u64 gp, const u32 win, u64* src) {
    u32 lo = 0, hi = A.n_sources;
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (A.src_off[mid] <= gp) lo = mid; else hi = mid;
    }
    *src = lo;
    return gp + win <= A.src_off[lo + 1];
}

// The wave's survivors as records: one add reserves room for all kHashes ballots', the first hash's first, each in lane order.
// The counter keeps counting past the capacity; nothing is written at or past it.  Every lane of the wave calls this.
template <u32 kHashes>
__device__ __forceinline__ void append_survivors(const HashArgs& A, const u32 lane, const bool keep[kHashes], const u64 h[kHashes], const u64 src) {
    unsigned long long have[kHashes];
    u32 n = 0;
#pragma unroll
    for (u32 i = 0; i < kHashes; ++i) n += (u32)__popcll(have[i] = __ballot(keep[i]));
    if (!n) return;   // (the whole wave)
    unsigned long long at = 0;
    if (lane == 0) at = atomicAdd(&A.counters[0], (unsigned long long)n);
    const u32 at_lo = (u32)__shfl((int)(u32)at, 0), at_hi = (u32)__shfl((int)(u32)(at >> 32), 0);
    u64 base = ((u64)at_hi << 32) | at_lo;
#pragma unroll
    for (u32 i = 0; i < kHashes; ++i) {
        const u64 slot = base + (u64)__popcll(have[i] & ((1ull << lane) - 1));
        if (keep[i] && slot < A.capacity) A.recs[slot] = Rec{h[i], src};
        base += (u64)__popcll(have[i]);
    }
}

#ifndef KSP_SKETCH_PARTS_ONLY   // (classify.hip takes the parts above and brings its own frame: classify_kernels.hip.h)
// The frame.  s_mask: kMaskWords of LDS; win: the positions of a window.  stage(c, w) puts the 16 bytes w of piece c into the
// kernel's LDS and returns their break bits; hashes(p, h) writes the kHashes hashes of the unbroken window at tile position p.
template <u32 kHashes, class Stage, class Hashes>
__device__ __forceinline__ void sketch_tiles(const HashArgs& A, const u32 win, u64* s_mask, Stage stage, Hashes hashes) {
    const u32 tid = threadIdx.x, lane = tid & 63;
    u32 n_bases = 0, n_valid = 0;
    for (u64 tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
        const u64 t0 = tile * kTile;
        // ---- the tile and its halo in LDS
        for (u32 c = tid; c < kChunks; c += kThreads) {   // (two trips for the first four threads, one for the others)
            u32 w[4];
            load_piece(A.seq, A.n_bytes, t0 + 16ull * c, w);
            const u32 breaks = stage(c, w);
            reinterpret_cast<uint16_t*>(s_mask)[c] = (uint16_t)breaks;
            if (c < kTile / 16) n_bases += 16u - (u32)__popc(breaks);   // (the tile's bases: the halo's are the next tile's)
        }
        __syncthreads();
        // ---- the positions of the tile
        for (u32 p = tid; p < kTile; p += kThreads) {   // (the same trips for every thread)
            bool keep[kHashes], pass = false;
            u64 h[kHashes], src = 0;
#pragma unroll
            for (u32 i = 0; i < kHashes; ++i) { keep[i] = false; h[i] = 0; }
            if (window_unbroken(s_mask, p, win)) {
                ++n_valid;
                hashes(p, h);
#pragma unroll
                for (u32 i = 0; i < kHashes; ++i) pass |= h[i] <= A.max_hash;
                if (pass) {
                    const bool inside = window_in_source(A, t0 + p, win, &src);   // (t0 + p < n_bytes: the window is unbroken)
#pragma unroll
                    for (u32 i = 0; i < kHashes; ++i) keep[i] = inside && h[i] <= A.max_hash;
                }
            }
            append_survivors<kHashes>(A, lane, keep, h, src);
        }
        __syncthreads();   // (the next tile's pieces overwrite the words)
    }
    n_bases = wave_sum(n_bases);
    n_valid = wave_sum(n_valid);
    if (lane == 0) {
        if (n_bases) atomicAdd(&A.counters[1], (unsigned long long)n_bases);
        if (n_valid) atomicAdd(&A.counters[2], (unsigned long long)n_valid);
    }
}

template <bool kWide>
__global__ __launch_bounds__(kThreads) void k_sketch_hash(const HashArgs A) {
    __shared__ u64 s_code[kCodeWords];
    __shared__ u64 s_mask[kMaskWords];
    sketch_tiles<1>(
        A, A.k, s_mask, [&](const u32 c, u32 w[4]) { return stage_bases(w, c, s_code); },
        [&](const u32 p, u64 h[1]) { h[0] = sk::kmer_hash(sk::canonical(kmer_at<kWide>(s_code, p, A.k), A.k), A.k, A.seed); });
}

__global__ __launch_bounds__(kThreads) void k_sketch_hash_protein(const MolArgs M) {
    __shared__ alignas(16) u32 s_letter[kLetterWords];   // little-endian: position i of the tile is byte i
    __shared__ u64 s_mask[kMaskWords];
    __shared__ uint8_t s_class[256];   // byte value -> letter, 0 for a break
    const HashArgs& A = M.h;
    const u32 n_words = (A.k + 7) / 8;   // 64-bit words of a k-mer's letters
    s_class[threadIdx.x] = (uint8_t)sk::residue_letter(M.mol, threadIdx.x);
    __syncthreads();
    sketch_tiles<1>(
        A, A.k, s_mask,
        [&](const u32 c, u32 w[4]) {
            u32 breaks = 0;
#pragma unroll
            for (u32 q = 0; q < 4; ++q) {
                u32 letters = 0;
#pragma unroll
                for (u32 j = 0; j < 4; ++j) {
                    const u32 l = s_class[(w[q] >> (8 * j)) & 0xFFu];
                    letters |= l << (8 * j);
                    breaks |= (l ? 0u : 1u) << (4 * q + j);
                }
                w[q] = letters;
            }
            *reinterpret_cast<uint4*>(&s_letter[4 * c]) = make_uint4(w[0], w[1], w[2], w[3]);
            return breaks;
        },
        [&](const u32 p, u64 h[1]) {
            const u32 w0 = p >> 2, sh = 8 * (p & 3);
            u64 w[8];
            u32 prev = s_letter[w0];
#pragma unroll
            for (u32 i = 0; i < 8; ++i) {   // (w0 + 2 n_words <= 1023 + 16: the last word of the halo)
                w[i] = 0;
                if (i < n_words) {
                    const u32 a = s_letter[w0 + 2 * i + 1], b = s_letter[w0 + 2 * i + 2];
                    const u32 lo = __funnelshift_r(prev, a, sh), hi = __funnelshift_r(a, b, sh);
                    prev = b;
                    const u32 bytes = A.k - 8 * i;   // (1 or more: i < n_words)
                    w[i] = sk::low_bytes(((u64)hi << 32) | lo, bytes);
                }
            }
            h[0] = sk::letters_hash<8>(w, A.k, A.seed);
        });
}

__global__ __launch_bounds__(kThreads) void k_sketch_hash_translated(const MolArgs M) {
    __shared__ u64 s_code[kCodeWords];
    __shared__ u64 s_mask[kMaskWords];
    __shared__ uint8_t s_codon[64];   // packed codon -> letter
    const HashArgs& A = M.h;
    const u32 k3 = 3 * A.k;   // the window: 3 .. 63 bases
    if (threadIdx.x < 64) s_codon[threadIdx.x] = (uint8_t)sk::codon_letter(M.mol, threadIdx.x);
    __syncthreads();
    sketch_tiles<2>(
        A, k3, s_mask, [&](const u32 c, u32 w[4]) { return stage_bases(w, c, s_code); },
        [&](const u32 p, u64 h[2]) {   // [0] the forward strand's, [1] the reverse strand's
            const sk::Kmer fw = kmer_at<true>(s_code, p, k3);
            u64 w[3];
            sk::translate_words(fw, A.k, s_codon, w);
            h[0] = sk::letters_hash<3>(w, A.k, A.seed);
            sk::translate_words(sk::reverse_complement(fw, k3), A.k, s_codon, w);
            h[1] = sk::letters_hash<3>(w, A.k, A.seed);
        });
}
#endif
