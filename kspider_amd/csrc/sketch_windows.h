// The rolling window of the host loops over DNA bytes (sketch_cpu.cpp: the DNA and the translated sketch; classify_cpu.cpp), over
// the arithmetic of sketch_hash.h.  Host only.
#ifndef KSPIDER_SKETCH_WINDOWS_H
#define KSPIDER_SKETCH_WINDOWS_H
#include <cstdint>

#include "sketch_hash.h"

namespace ksp_sketch {

// full(left) for every `win` (1 .. 64) consecutive bases among the bytes [first, last), `left` being them left-aligned; a byte
// that is no base starts the window over.
template <class Full>
void each_base_window(const uint8_t* seq, const uint64_t first, const uint64_t last, const unsigned win, Full full) {
    Kmer fw{0, 0};       // the last min(have, win) bases, right-aligned
    unsigned have = 0;   // bases since the last break, capped at win
    for (uint64_t p = first; p < last; ++p) {
        const unsigned c = seq[p];
        if (!is_base(c)) { have = 0; fw = Kmer{0, 0}; continue; }
        fw = shift_left(fw, 2);
        fw.lo |= base_code(c);
        if (have < win) ++have;
        if (have == win) full(shift_left(fw, 128 - 2 * win));   // (drops the bases older than win)
    }
}

}  // namespace ksp_sketch
#endif
