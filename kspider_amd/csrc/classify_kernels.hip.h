// The hash pass of classify; included into classify.hip's anonymous namespace behind sketch_kernels.hip.h and
// query_table.hip.h.  k_classify_hash is k_sketch_hash with another sink: the same tile staging, break mask, kmer_at and
// window_in_source, but a survivor (hash, segment) does not go to HBM: the wave compacts its survivors by ballot into a list in
// LDS, and when the list could not take another round of positions — and once more at the end — the workgroup drains it: every
// lane takes kProbeKeys survivors and runs query_lookup on them together, so that the dependent loads of several look-ups are in
// flight, and only a hit leaves the workgroup, as (record << 32) | table_index with one returning add per wave.  The list lives
// across tiles: at a real `scaled` a tile has a handful of survivors, and a drain per tile would look them up one chain at a time.
//
// LDS: s_code 1 040 + s_mask 520 bytes (the sketcher's), s_hash 16 KiB + s_seg 8 KiB (the list: kListCap = 2 048 entries),
// s_count 4.  A round is kRound = 1 024 positions (four trips of the workgroup), so a round appends at most kRound entries, and
// the list is drained when it holds more than kListCap - kRound: with max_hash = 2^64 - 1 and no break byte that is after every
// second round, the list then holding exactly kListCap entries.  The decision is the OR over the workgroup of "my wave's last reservation ended above the
// mark" — the wave that reserved last saw the final count —, taken by the barrier that ends the round, so it is uniform without a
// second barrier.
constexpr u32 kRound = 4 * kThreads;
constexpr u32 kListCap = 2 * kRound;
static_assert(kTile % kRound == 0 && kRound == kThreads * (u32)kProbeKeys, "a drain step gives every lane kProbeKeys entries");

struct ClassifyArgs {
    HashArgs h;               // recs / capacity unused; counters: [0] hit words, the ones without room included, [1] bases,
                              // [2] windows without a break, [3] kept windows
    QTable T;                 // the references' table; T.nq = 0: there is none, nothing is looked up
    const u32* seg_rec;       // the record of every segment
    u32* kept_windows;        // per record
    unsigned long long* hits; // room for hit_capacity words
    u64 hit_capacity;
    u32 tally;                // 0: the batch runs again — only the hit words are produced, nothing else is counted
};

// The list's first n entries: their records' kept windows counted, their hashes looked up, the hits appended.  Every lane of the
// workgroup calls this with the same n; nobody appends to the list meanwhile.
__device__ __forceinline__ void classify_drain(const ClassifyArgs& C, const u64* s_hash, const u32* s_seg, const u32 n, u32& n_kept) {
    const u32 tid = threadIdx.x, lane = tid & 63;
    for (u32 e0 = 0; e0 < n; e0 += kRound) {   // (the same trips for every lane)
        u64 k[kProbeKeys];
        bool live[kProbeKeys];
        u32 at[kProbeKeys], rec[kProbeKeys];
#pragma unroll
        for (int x = 0; x < kProbeKeys; ++x) {
            const u32 e = e0 + (u32)x * kThreads + tid;
            live[x] = e < n;
            k[x] = live[x] ? s_hash[e] : 0;
            rec[x] = live[x] ? C.seg_rec[s_seg[e]] : 0;
            at[x] = 0;
        }
        if (C.tally) {
#pragma unroll
            for (int x = 0; x < kProbeKeys; ++x)
                if (live[x]) { atomicAdd(&C.kept_windows[rec[x]], 1u); ++n_kept; }
        }
        if (C.T.nq) {
            query_lookup(C.T, k, live, at);
        } else {
#pragma unroll
            for (int x = 0; x < kProbeKeys; ++x) live[x] = false;
        }
        // ---- the hits: one add reserves room for the four ballots', the first key's first, each in lane order
        unsigned long long have[kProbeKeys];
        u32 n_hit = 0;
#pragma unroll
        for (int x = 0; x < kProbeKeys; ++x) n_hit += (u32)__popcll(have[x] = __ballot(live[x]));
        if (!n_hit) continue;   // (the whole wave)
        unsigned long long first = 0;
        if (lane == 0) first = atomicAdd(&C.h.counters[0], (unsigned long long)n_hit);
        const u32 lo = (u32)__shfl((int)(u32)first, 0), hi = (u32)__shfl((int)(u32)(first >> 32), 0);
        u64 base = ((u64)hi << 32) | lo;
#pragma unroll
        for (int x = 0; x < kProbeKeys; ++x) {
            const u64 slot = base + (u64)__popcll(have[x] & ((1ull << lane) - 1));
            if (live[x] && slot < C.hit_capacity) C.hits[slot] = ((u64)rec[x] << 32) | at[x];
            base += (u64)__popcll(have[x]);
        }
    }
}

template <bool kWide>
__global__ __launch_bounds__(kThreads) void k_classify_hash(const ClassifyArgs C) {
    __shared__ u64 s_code[kCodeWords];
    __shared__ u64 s_mask[kMaskWords];
    __shared__ u64 s_hash[kListCap];
    __shared__ u32 s_seg[kListCap];
    __shared__ u32 s_count;
    const HashArgs& A = C.h;
    const u32 tid = threadIdx.x, lane = tid & 63, win = A.k;
    u32 n_bases = 0, n_valid = 0, n_kept = 0;
    u32 wave_end = 0;   // where the wave's last reservation in the list ended (the same in all its lanes)
    if (tid == 0) s_count = 0;
    for (u64 tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
        const u64 t0 = tile * kTile;
        // ---- the tile and its halo in LDS, as in sketch_tiles
        for (u32 c = tid; c < kChunks; c += kThreads) {
            u32 w[4];
            load_piece(A.seq, A.n_bytes, t0 + 16ull * c, w);
            const u32 breaks = stage_bases(w, c, s_code);
            reinterpret_cast<uint16_t*>(s_mask)[c] = (uint16_t)breaks;
            if (c < kTile / 16) n_bases += 16u - (u32)__popc(breaks);
        }
        __syncthreads();
        // ---- the positions of the tile, a round at a time
        for (u32 r0 = 0; r0 < kTile; r0 += kRound) {
            for (u32 p = r0 + tid; p < r0 + kRound; p += kThreads) {   // (the same trips for every thread)
                bool keep = false;
                u64 h = 0, src = 0;
                if (window_unbroken(s_mask, p, win)) {
                    ++n_valid;
                    h = sk::kmer_hash(sk::canonical(kmer_at<kWide>(s_code, p, win), win), win, A.seed);
                    if (h <= A.max_hash) keep = window_in_source(A, t0 + p, win, &src);   // (t0 + p < n_bytes: the window is unbroken)
                }
                const unsigned long long have = __ballot(keep);
                if (!have) continue;   // (the whole wave)
                u32 first = 0;
                if (lane == 0) first = atomicAdd(&s_count, (u32)__popcll(have));
                first = (u32)__shfl((int)first, 0);
                if (keep) {   // (first + popc(have) <= kListCap: the list held at most kListCap - kRound when the round began)
                    const u32 slot = first + (u32)__popcll(have & ((1ull << lane) - 1));
                    s_hash[slot] = h;
                    s_seg[slot] = (u32)src;
                }
                wave_end = first + (u32)__popcll(have);
            }
            // the round's appends are done, and after the tile's last round the next tile's pieces may overwrite the words
            if (__syncthreads_or(wave_end > kListCap - kRound)) {
                classify_drain(C, s_hash, s_seg, s_count, n_kept);
                __syncthreads();
                if (tid == 0) s_count = 0;
                wave_end = 0;
                __syncthreads();
            }
        }
    }
    __syncthreads();   // (a workgroup without a tile: s_count = 0 is visible)
    classify_drain(C, s_hash, s_seg, s_count, n_kept);
    if (!C.tally) return;
    n_bases = wave_sum(n_bases);
    n_valid = wave_sum(n_valid);
    n_kept = wave_sum(n_kept);
    if (lane == 0) {
        if (n_bases) atomicAdd(&A.counters[1], (unsigned long long)n_bases);
        if (n_valid) atomicAdd(&A.counters[2], (unsigned long long)n_valid);
        if (n_kept) atomicAdd(&A.counters[3], (unsigned long long)n_kept);
    }
}
