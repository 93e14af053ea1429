// The hash passes of the protein, dayhoff and hp sketches; included into sketcher.hip behind k_sketch_hash, whose
// shape both keep: a workgroup of 256 loops over tiles of kTile positions, every thread loads 16 bytes (the first four another 16:
// the halo of 64 bytes), bytes behind the stream's end are breaks, a survivor finds its source by binary search, is dropped when
// its window would cross the source's end, and is appended as (hash, source) with one returning add per wave.
//   k_sketch_hash_protein     the bytes are residues.  The tile sits in LDS as the letters that are hashed, one byte per position
//                             (0 for a break), beside the break bits.  A lane reads the 32-bit words its k letters lie in —
//                             neighbouring lanes read neighbouring or the same words: no bank is asked for two addresses — and
//                             funnel-shifts them down by its byte offset, masks the tail, hashes.
//   k_sketch_hash_translated  the bytes are DNA, staged exactly as in k_sketch_hash; the window is 3k bases.  The forward k-mer
//                             and its reverse complement are each translated codon by codon through a 64-byte LDS table and
//                             hashed: two possible survivors per position, appended with two ballots and one add.
// The arithmetic is sketch_mol.h, shared with the host loop.

struct MolArgs {
    HashArgs h;   // k: residues per k-mer
    int mol;      // KSP_MOL_PROTEIN / _DAYHOFF / _HP
};

constexpr u32 kLetterWords = (kTile + 64) / 4;   // the tile's and the halo's letters as 32-bit words

// the source of stream position gp (the last s with src_off[s] <= gp), and whether a window of `win` bytes at gp ends inside it
__device__ inline bool window_in_source(const HashArgs& A, const u64 gp, const u32 win, u64* src) {
    u32 lo = 0, hi = A.n_sources;
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (A.src_off[mid] <= gp) lo = mid; else hi = mid;
    }
    *src = lo;
    return gp + win <= A.src_off[lo + 1];
}

// 16 bytes of the stream at `at` as four words; bytes at and behind n_bytes are 0
__device__ inline void load_piece(const uint8_t* seq, const u64 n_bytes, const u64 at, u32 w[4]) {
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

__global__ __launch_bounds__(kThreads) void k_sketch_hash_protein(const MolArgs M) {
    __shared__ alignas(16) u32 s_letter[kLetterWords];   // little-endian: position i of the tile is byte i
    __shared__ u64 s_mask[kMaskWords];       // bit i of word m = position 64m + i is a break
    __shared__ uint8_t s_class[256];         // byte value -> letter, 0 for a break
    const HashArgs& A = M.h;
    const u32 tid = threadIdx.x, lane = tid & 63;
    u32 n_bases = 0, n_valid = 0;
    const u64 win_mask = A.k == 64 ? ~0ull : (1ull << A.k) - 1;
    const u32 n_words = (A.k + 7) / 8;   // 64-bit words of a k-mer's letters
    s_class[tid] = (uint8_t)sk::residue_letter(M.mol, tid);
    __syncthreads();
    for (u64 tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
        const u64 t0 = tile * kTile;
        // ---- the tile and its halo as letters and break bits
        for (u32 c = tid; c < kChunks; c += kThreads) {   // (two trips for the first four threads, one for the others)
            u32 w[4];
            load_piece(A.seq, A.n_bytes, t0 + 16ull * c, w);
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
            reinterpret_cast<uint16_t*>(s_mask)[c] = (uint16_t)breaks;
            if (c < kTile / 16) n_bases += 16u - (u32)__popc(breaks);
        }
        __syncthreads();
        // ---- the positions of the tile
        for (u32 p = tid; p < kTile; p += kThreads) {   // (the same trips for every thread)
            const u32 m = p >> 6, s = p & 63;
            const u64 window = s ? (s_mask[m] >> s) | (s_mask[m + 1] << (64 - s)) : s_mask[m];   // (m + 1 <= 64: the halo's word)
            const bool valid = (window & win_mask) == 0;
            bool keep = false;
            u64 h = 0, src = 0;
            if (valid) {
                ++n_valid;
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
                h = sk::letters_hash<8>(w, A.k, A.seed);
                if (h <= A.max_hash) keep = window_in_source(A, t0 + p, A.k, &src);   // (t0 + p < n_bytes: the window is valid)
            }
            const unsigned long long have = __ballot(keep);
            if (!have) continue;   // (the whole wave)
            const int first = __ffsll((long long)have) - 1;
            unsigned long long at = 0;
            if ((int)lane == first) at = atomicAdd(&A.counters[0], (unsigned long long)__popcll(have));
            const u32 at_lo = (u32)__shfl((int)(u32)at, first), at_hi = (u32)__shfl((int)(u32)(at >> 32), first);
            const u64 slot = (((u64)at_hi << 32) | at_lo) + (u64)__popcll(have & ((1ull << lane) - 1));
            if (keep && slot < A.capacity) A.recs[slot] = Rec{h, src};
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

__global__ __launch_bounds__(kThreads) void k_sketch_hash_translated(const MolArgs M) {
    __shared__ u64 s_code[kCodeWords];   // big-endian: base 32j of the tile on top of word j
    __shared__ u64 s_mask[kMaskWords];   // little-endian: bit i of word m = position 64m + i is a break
    __shared__ uint8_t s_codon[64];      // packed codon -> letter
    const HashArgs& A = M.h;
    const u32 tid = threadIdx.x, lane = tid & 63;
    u32 n_bases = 0, n_valid = 0;
    const u32 k3 = 3 * A.k;   // the window: 3 .. 63 bases
    const u64 win_mask = (1ull << k3) - 1;
    if (tid < 64) s_codon[tid] = (uint8_t)sk::codon_letter(M.mol, tid);
    __syncthreads();
    for (u64 tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
        const u64 t0 = tile * kTile;
        // ---- the tile and its halo as codes and break bits
        for (u32 c = tid; c < kChunks; c += kThreads) {   // (two trips for the first four threads, one for the others)
            u32 w[4];
            load_piece(A.seq, A.n_bytes, t0 + 16ull * c, w);
            u32 code = 0, breaks = 0;
#pragma unroll
            for (u32 j = 0; j < 16; ++j) {
                const u32 b = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                code |= sk::base_code(b) << (30 - 2 * j);
                breaks |= (sk::is_base(b) ? 0u : 1u) << j;
            }
            reinterpret_cast<u32*>(s_code)[c ^ 1u] = code;   // (the even piece is the upper half of its word)
            reinterpret_cast<uint16_t*>(s_mask)[c] = (uint16_t)breaks;
            if (c < kTile / 16) n_bases += 16u - (u32)__popc(breaks);
        }
        __syncthreads();
        // ---- the positions of the tile
        for (u32 p = tid; p < kTile; p += kThreads) {   // (the same trips for every thread)
            const u32 m = p >> 6, s = p & 63;
            const u64 window = s ? (s_mask[m] >> s) | (s_mask[m + 1] << (64 - s)) : s_mask[m];   // (m + 1 <= 64: the halo's word)
            const bool valid = (window & win_mask) == 0;
            bool keep_f = false, keep_r = false;
            u64 h_f = 0, h_r = 0, src = 0;
            if (valid) {
                ++n_valid;
                const u32 j = p >> 5, s2 = 2 * (p & 31);
                sk::Kmer fw;
                fw.hi = s2 ? (s_code[j] << s2) | (s_code[j + 1] >> (64 - s2)) : s_code[j];
                fw.lo = s2 ? (s_code[j + 1] << s2) | (s_code[j + 2] >> (64 - s2)) : s_code[j + 1];   // (j + 2 <= 129)
                fw = sk::keep_top(fw, k3);
                const sk::Kmer rc = sk::reverse_complement(fw, k3);
                u64 w[3];
                sk::translate_words(fw, A.k, s_codon, w);
                h_f = sk::letters_hash<3>(w, A.k, A.seed);
                sk::translate_words(rc, A.k, s_codon, w);
                h_r = sk::letters_hash<3>(w, A.k, A.seed);
                if (h_f <= A.max_hash || h_r <= A.max_hash) {
                    const bool inside = window_in_source(A, t0 + p, k3, &src);   // (t0 + p < n_bytes: the window is valid)
                    keep_f = inside && h_f <= A.max_hash;
                    keep_r = inside && h_r <= A.max_hash;
                }
            }
            const unsigned long long have_f = __ballot(keep_f), have_r = __ballot(keep_r);
            if (!(have_f | have_r)) continue;   // (the whole wave)
            // one add for both strands' survivors: the forward ones first, then the reverse ones, each in lane order
            const u32 n_f = (u32)__popcll(have_f);
            unsigned long long at = 0;
            if (lane == 0) at = atomicAdd(&A.counters[0], (unsigned long long)(n_f + (u32)__popcll(have_r)));
            const u32 at_lo = (u32)__shfl((int)(u32)at, 0), at_hi = (u32)__shfl((int)(u32)(at >> 32), 0);
            const u64 base = ((u64)at_hi << 32) | at_lo, below = (1ull << lane) - 1;
            const u64 slot_f = base + (u64)__popcll(have_f & below), slot_r = base + n_f + (u64)__popcll(have_r & below);
            if (keep_f && slot_f < A.capacity) A.recs[slot_f] = Rec{h_f, src};
            if (keep_r && slot_r < A.capacity) A.recs[slot_r] = Rec{h_r, src};
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
