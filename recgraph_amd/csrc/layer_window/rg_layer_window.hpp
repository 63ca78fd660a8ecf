// The column window of the windowed layer rebuild (layer_window/rg_layer_window.hip): ONE statement of where the window of a
// layer row lies, read by the kernel that fills it, by k_trace (rg_pathwise.hip) that walks it, and by the host check
// (tests/c/layer_window_check.cpp: plain C++, no HIP).
//
// The traceback walks from its start cell (layer row t_start, column start_col) towards row 0 and column 0; an alignment without
// indels walks the diagonal through the start cell.  The window of layer row t is W columns around that diagonal:
//   centre(t) = start_col - (t_start - t),   left(t) = clamp(centre(t) - W / 2, 0, wpad - W) rounded down to a multiple of 4
// (4 columns = one byte of the layer buffer, and a multiple of both column-block widths, 2 and 4).  left() is monotone in t, moves
// by at most 4 columns from one row to the next, and the start cell lies inside the window of its own row.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RG_LW_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RG_LW_HD inline
#endif

namespace rg {

// internal status bit (masked out of every record like ST_RETRY): the walk of this read left the column window, or met a decision
// whose inputs the window did not hold; the full-width layer kernels and a second k_trace rebuild and walk it
constexpr uint32_t ST_LAYER_FULL = 0x400u;
// word of the chunk's need[] read-back that counts those reads
constexpr int NEED_LAYER_FULL = 5;

// prefix of the pseudo-statistic that names the windowed kernel a batch launched ("mem:layer_window:rg::k_layer_win<16, 4>": ms 0,
// launches counted; always reported, like "mem:layer_full_reads" — "inst:" is the optional log of the kernels of csrc/*.hip)
constexpr const char* LAYER_WINDOW_LOG = "mem:layer_window:";

constexpr int LAYER_WINDOW_DEFAULT = 256;      // columns: 64 lanes x 4
constexpr int LAYER_WINDOW_NARROW = 128;       // 64 lanes x 2

// W: window width in columns (a multiple of 64, <= wpad); wpad: padded columns of a row (64 x columns per lane)
RG_LW_HD int layer_window_left(int start_col, int t_start, int t, int W, int wpad) {
    int e = start_col - (t_start - t) - W / 2;
    const int hi = wpad - W;
    e = e > hi ? hi : e;
    e = e < 0 ? 0 : e;
    return e & ~3;
}

// Index of `row` among the rows list[0 .. nr) of a path (ascending in the forward lists, descending in the reverse ones), -1 if
// the path does not visit it.
RG_LW_HD int layer_row_index(const int* list, int nr, int row, bool descending) {
    int lo = 0, hi = nr - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const int r = list[mid];
        if (r == row) return mid;
        if (descending ? r > row : r < row) lo = mid + 1;
        else hi = mid - 1;
    }
    return -1;
}

// Unknown values: a cell whose chain of sources leaves the window holds a sentinel below every real value.  The packed rows of
// a batch that takes the windowed kernel hold real values >= LAYER_WINDOW_ZLO (plan_pathwise checks it), one step changes a
// value by at most 2000 (sweep16_admissible: entries <= 1000 in magnitude), and the kernel puts every value below
// LAYER_WINDOW_KNOWN back to the sentinel after every row: real + step >= -26000 > KNOWN > -28000 >= sentinel + step.
constexpr int LAYER_WINDOW_UNKNOWN = -30000;   // = the "minus infinity" of the packed rows (columns outside the read)
constexpr int LAYER_WINDOW_KNOWN = -27000;
constexpr int LAYER_WINDOW_ZLO = -24000;

}  // namespace rg
