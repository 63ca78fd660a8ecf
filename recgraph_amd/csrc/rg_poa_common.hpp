// The skeleton the POA kernels share (rg_poa.hip, rg_poa_banded.hip, rg_poa_local.hip): one wave per read, rows sequential, the
// left recurrence as a wave prefix scan, a one-lane traceback.  Only __device__ __forceinline__ functions and small structs:
// every kernel inlines what it uses, and its .hip file holds what the mode does differently.  What is NOT here: the registers
// that carry the previous row (named registers / select chains with empty asm statements) — their exact form is what keeps
// them out of scratch, see the comments in the kernels.
#pragma once
#include "rg_device.hpp"
#include "rg_poa_args.hpp"

namespace rg {

constexpr int GAP = 5;                        // '-' in the 6 x 6 score table
constexpr int NEG = INT32_MIN / 4;            // "no value" of the scans: survives one addition of a score
constexpr uint32_t X_BIT = 0x80000000u;       // w0: the cell's left neighbour continues a gap (path_x = 'X')

// direction codes of bitfield_path.rs:3-15 in the low 3 bits of a path word w0 = pred << 3 | dir | X << 31; w1 = predY << 1 | Y.
// 0 doubles as the f32 path value 0.0 of the AVX2 local flavour.
enum : uint32_t { PD_O = 0, PD_D = 1, PD_d = 2, PD_L = 3, PD_U = 4 };

// ---- prologue -----------------------------------------------------------------------------------------------------------------
// Score table and (when it fits) the read's base codes live in LDS: both are indexed per lane every row, and as kernel-argument /
// global loads each lookup was a dependent memory round trip (78 % of the wave cycles waiting).  The LDS array is declared by the
// kernel: [36 ints | max_n + 2 bytes when a.lds_read].
template <bool kLdsRead>
struct PoaRead {
    int slot, rd, lane;       // arena slot of this launch, read of the batch
    int n, W;                 // bases, columns (n + 1)
    const uint8_t* gread;     // at(j), j = 1..n
    const uint8_t* lread;
    const int* sct;           // [36]
    DevRecord* rec;
    int *am, *ay;             // score planes of this read (ay: second plane of the affine modes)
    uint32_t *pw0, *pw1;      // path word planes
    // (kLdsRead is a template argument: a run-time choice between the two pointers would turn every access into a FLAT load)
    __device__ __forceinline__ int at(int j) const { return kLdsRead ? (int)lread[j] : (int)gread[j]; }
    // false: the read has a base outside ACGTN, its record is written and the wave returns
    __device__ __forceinline__ bool init(const PoaArgs& a, int* lds, int planes) {
        slot = blockIdx.x;
        rd = a.read_base + slot;
        lane = threadIdx.x;
        const long long ro = a.read_off[rd];
        n = (int)(a.read_off[rd + 1] - ro);
        W = n + 1;
        gread = a.reads + ro - 1;
        uint8_t* lr = reinterpret_cast<uint8_t*>(lds + 36);
        if (lane < 36) lds[lane] = a.sc.t[lane];
        if (kLdsRead)
            for (int j = 1 + lane; j <= n; j += WAVE) lr[j] = gread[j];
        __syncthreads();
        sct = lds;
        lread = lr;
        rec = a.rec + rd;
        if (a.bad[rd]) {
            if (lane == 0) { rec->status = ST_BAD_BASE; rec->n_ops = 0; rec->score = 0; }
            return false;
        }
        am = a.arena_m + (long long)slot * a.cap_cells * planes;
        ay = am + a.cap_cells;
        pw0 = a.arena_pw + (long long)slot * a.cap_cells * planes;
        pw1 = pw0 + a.cap_cells;
        return true;
    }
};

inline size_t poa_lds_bytes(const PoaArgs& a) {
    return 36 * sizeof(int) + (a.lds_read ? (((size_t)a.max_n + 2 + 3) & ~(size_t)3) : 0);
}
// one wave per read; TA_LDS / TA_GLOBAL: the template arguments of the instantiation with the read in LDS / in global memory
#define RG_POA_LAUNCH(K, TA_LDS, TA_GLOBAL, a, s)                                                        \
    do {                                                                                                 \
        if ((a).lds_read) RG_LAUNCH(K, TA_LDS, dim3((a).nreads), dim3(WAVE), poa_lds_bytes(a), s, a);    \
        else RG_LAUNCH(K, TA_GLOBAL, dim3((a).nreads), dim3(WAVE), poa_lds_bytes(a), s, a);              \
    } while (0)

// ---- scan steps ---------------------------------------------------------------------------------------------------------------
// Linear gaps: v[c] = max(b[c], v[c-1] + g[c]).  With G the prefix sum of g, z = v - G turns the chain into a prefix max
// (DESIGN.md "m0 left sweep as a scan").  One 64-column chunk: `b` is the cell's value without the chain (`fill` on idle lanes),
// G its inclusive gap sum; zprev + G is the chain's value at this lane and zprev > y (or >=, the caller's rule) says it wins.
struct LinScan { int y, zi, zprev; };
__device__ __forceinline__ LinScan lin_scan(int b, int G, bool act, int fill, int lane, int carry_z) {
    const int y = act ? b - G : fill;
    const int zi = dpp_incl_max(y, fill);
    int zprev = dpp_shr1(zi, fill);
    zprev = lane == 0 ? carry_z : max(zprev, carry_z);
    return {y, zi, zprev};
}
// the carries behind a chunk: carry_z is updated, the next carry_G (G of the chunk's last lane) is returned
__device__ __forceinline__ int lin_carry(const LinScan& s, int G, int& carry_z) {
    carry_z = max(carry_z, __builtin_amdgcn_readlane(s.zi, WAVE - 1));
    return __builtin_amdgcn_readlane(G, WAVE - 1);
}

// Affine gaps: x[j] = e + max(x[j-1], m[j-1] + o)  =>  x[j] - e*j = max_{k<j} (src[k] - e*k)  (o <= 0).  The step itself stays in the
// two kernels (through a shared function with the mode's rule for x passed in, k_poa_banded<true> took 86 VGPRs instead of 84);
// shared are its state and its carries: zi the inclusive prefix max of src - e*col, xval the lane's x, xprev / tprev x and t of
// the column to the left (from the carries in lane 0) for the X flag.
struct AffCarry { int z, x, t; };
struct AffScan { int zi, xval, xprev, tprev; };
__device__ __forceinline__ void aff_carry(const AffScan& s, int tcur, AffCarry& k) {
    k.x = __builtin_amdgcn_readlane(s.xval, WAVE - 1);     // x of the chunk's last column
    k.t = __builtin_amdgcn_readlane(tcur, WAVE - 1);
    k.z = max(k.z, __builtin_amdgcn_readlane(s.zi, WAVE - 1));
}

// ---- the (d, u, l) decision of utils.rs:129-140: D on ties, then U, then L ---------------------------------------------------------
struct Cell { int v; uint32_t w; };
__device__ __forceinline__ Cell pick_dul(int dv, int uu, int l, uint32_t wd, uint32_t wu, uint32_t wl) {
    if (dv < uu) return uu < l ? Cell{l, wl} : Cell{uu, wu};
    return dv < l ? Cell{l, wl} : Cell{dv, wd};
}

// ---- one-lane walkers ----------------------------------------------------------------------------------------------------------
// A walker follows path words from the end cell to an 'O' cell and writes one op per step.  How a cell is addressed is a policy:
//   width(row)              columns the row stores;
//   w0 / w1(row, col)       its path words;
//   in_run(row, col)        a gap run may read (row, col) (full width: the run cannot leave the row);
//   row_ok(p)               a Y word may name row p;
//   pred_col(row, col, p, out)  the position of column `col` in row p; false = the reference's usize arithmetic wraps.
struct SameColumn {           // rows are stored by absolute column (all that walk_step needs: k_m0_simd)
    __device__ __forceinline__ bool pred_col(int, int col, int, int& out) const { out = col; return true; }
};
struct FullWidth : SameColumn {   // row * W + col (local modes)
    const uint32_t *pw0, *pw1;
    int W, L;
    static constexpr uint32_t kPredMask = 0xfffffu;
    __device__ __forceinline__ int width(int) const { return W; }
    __device__ __forceinline__ uint32_t w0(int row, int col) const { return pw0[(long long)row * W + col]; }
    __device__ __forceinline__ uint32_t w1(int row, int col) const { return pw1[(long long)row * W + col]; }
    __device__ __forceinline__ bool in_run(int, int) const { return true; }
    __device__ __forceinline__ bool row_ok(int p) const { return p < L - 1; }
};
struct BandRel {              // cell j of row i <-> absolute column left_i + j, rinfo[i] = {arena offset, left, right, best}
    const uint32_t *pw0, *pw1;
    const int4* rinfo;
    static constexpr uint32_t kPredMask = 0xffffu;
    __device__ __forceinline__ int width(int row) const { const int4 q = rinfo[row]; return q.z - q.y; }
    __device__ __forceinline__ uint32_t w0(int row, int col) const { return pw0[rinfo[row].x + col]; }
    __device__ __forceinline__ uint32_t w1(int row, int col) const { return pw1[rinfo[row].x + col]; }
    __device__ __forceinline__ bool in_run(int row, int col) const { return col >= 0 && col < width(row); }
    __device__ __forceinline__ bool row_ok(int) const { return true; }
    // j_pos of the reference
    __device__ __forceinline__ bool pred_col(int row, int col, int pred, int& out) const {
        const int lr = rinfo[row].y, lp = rinfo[pred].y;
        if (lp < lr) { out = col + (lr - lp); return true; }
        if (col < lp - lr) return false;
        out = col - (lp - lr);
        return true;
    }
};

struct OpsOut {
    uint8_t* ops;
    int32_t* orow;
    long long cap;
    int n;
    __device__ __forceinline__ OpsOut(const PoaArgs& a, int rd)
        : ops(a.ops + (long long)rd * a.ops_stride), orow(a.oprows + (long long)rd * a.ops_stride), cap(a.ops_stride), n(0) {}
    __device__ __forceinline__ bool full() const { return n + 2 >= cap; }
    __device__ __forceinline__ void emit(uint32_t op, int row) { ops[n] = (uint8_t)op; orow[n] = row; ++n; }
};

// Every walker function returns false where the reference would panic (ST_WOULD_PANIC at the caller).
// One D / U / L step out of (row, col); dir is a PD_* code.
template <typename A>
__device__ __forceinline__ bool walk_step(const A& c, uint32_t dir, int pred, int& row, int& col, OpsOut& out) {
    int jp = 0;
    const bool jp_ok = c.pred_col(row, col, pred, jp);
    if (dir == PD_D || dir == PD_d) {
        if (!jp_ok || jp == 0) return false;
        out.emit(OP_D | (dir == PD_d ? 0x40 : 0), pred);
        row = pred; col = jp - 1;
    } else if (dir == PD_L) {
        if (col == 0) return false;
        out.emit(OP_L, -1);
        col -= 1;
    } else {
        if (!jp_ok) return false;
        out.emit(OP_U, pred);
        row = pred; col = jp;
    }
    return true;
}
// affine L run: left while the X bit is set; every op after the first continues the gap
template <typename A>
__device__ __forceinline__ bool walk_l_run(const A& c, int row, int& col, OpsOut& out) {
    for (bool first = true;; first = false) {
        if (!c.in_run(row, col)) return false;
        if (!(c.w0(row, col) >> 31)) return true;
        if (col == 0 || out.full()) return false;
        out.emit(OP_L | (first ? 0 : OP_CONT), -1);
        col -= 1;
    }
}
// affine U run: up through the Y words while the Y bit is set.  kEmit = false walks without writing ops (band_ampl_enough).
template <bool kEmit, typename A>
__device__ __forceinline__ bool walk_u_run(const A& c, int& row, int& col, OpsOut& out) {
    for (bool first = true;; first = false) {
        if (!c.in_run(row, col)) return false;
        const uint32_t y1 = c.w1(row, col);
        if (!(y1 & 1u)) return true;
        const int p = (int)(y1 >> 1);
        int jq;
        if (!c.row_ok(p) || !c.pred_col(row, col, p, jq) || (kEmit && out.full())) return false;
        if (kEmit) out.emit(OP_U | (first ? 0 : OP_CONT), p);
        col = jq; row = p;
    }
}
// The traceback of the modes with 3-bit direction codes (gaf_output.rs:124-213 / 280-344 / 404-453 / 527-598 / 662-717): from
// (row, col) to the 'O' cell where it leaves them.  Returns 0 or ST_WOULD_PANIC.
template <bool kAffine, typename A>
__device__ __forceinline__ uint32_t walk_trace(const A& c, int L, int W, int& row, int& col, OpsOut& out) {
    int guard = 0;
    while (true) {
        if (++guard > 4 * (L + W) || out.full()) return ST_WOULD_PANIC;
        if (row < 0 || row >= L - 1 || col < 0 || col >= c.width(row)) return ST_WOULD_PANIC;
        const uint32_t w = c.w0(row, col);
        const uint32_t dir = w & 7u;
        if (dir == PD_O) return 0;
        const int pred = (int)((w >> 3) & A::kPredMask);
        bool ok;
        if (kAffine && dir == PD_L && (w >> 31)) ok = walk_l_run(c, row, col, out);
        else if (kAffine && dir == PD_U && (c.w1(row, col) & 1u)) ok = walk_u_run<true>(c, row, col, out);
        else ok = dir <= PD_U && walk_step(c, dir, pred, row, col, out);
        if (!ok) return ST_WOULD_PANIC;
    }
}

// ---- epilogue -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void write_record(DevRecord* rec, uint32_t status, int score, int end_row, int end_col, int stop_row,
                                             int stop_col, int n_ops) {
    rec->status = status;
    rec->score = score;
    rec->fscore = (float)score;
    rec->end_row = end_row;
    rec->end_col = end_col;
    rec->stop_row = stop_row;
    rec->stop_col = stop_col;
    rec->n_ops = n_ops;
    rec->n_fwd_ops = 0;
}

}  // namespace rg
