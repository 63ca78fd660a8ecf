// k_layer16 (rg_sweep16.hip) inside a COLUMN WINDOW around the walk.
//
// k_layer16 rebuilds every row of the chosen path at every column and stores a 2-bit move per cell; k_trace then reads one move
// per step of its walk, at most rows + n of ~10^6.  This kernel keeps W = 64 x CW columns of the row — the window of
// layer_window_left (rg_layer_window.hpp), a diagonal band through the walk's start cell — and runs the same arithmetic on them:
// z-space rows, GI0 in column 0, the zero_prev quirk of the first reverse row, trace_score at the start cell.
//
// Why that is exact here although a band is not for the sweeps: the layer rebuild decides nothing.  Every cell takes
// the source the sweep's direction word names and adds one step, so a value depends on its chain of sources only.  A cell whose
// source lies outside the window is UNKNOWN — a sentinel below every real value, put back after every row so that it can neither
// drift up into the real range nor wrap — and the unknown spreads only along chains that really leave the window.  A decision is
// stored only when its three inputs (d, u, l) are known, else as code 0 (k_layer16 stores 1 = D, 2 = U, 3 = L); k_trace hands a
// read whose walk meets a 0 or leaves the window to the full-width kernels (ST_LAYER_FULL).
//
// Lanes: column block b = c / CW lives in lane b mod 64, so a shift of the window moves no data: the lane whose block left takes
// the entering one, resets its registers to unknown and fetches that block's base codes (LDS).  The left neighbour of lane 0 is
// lane 63 (a DPP wave rotate); the lane at the window's left edge reads unknown there.  A lane's registers are RowOps16's at
// H = CW / 2: register r holds column r of the block in its low half and column H + r in its high half.
//
// Direction words: the word of sweep lane c / C (C / CW window lanes share one: a row reads 64 bytes at C = 16, not 256).  Output: the
// CW decisions of a lane are CW / 4 bytes of the layer buffer at the place the full-width layout gives those columns; bytes
// outside the window are neither written here nor read by k_trace.
#include "rg_layer_window.hpp"

#include "../rg_path_kernels.hpp"
#include "../rg_pk16.hpp"

namespace rg {

namespace {

constexpr int UNK = LAYER_WINDOW_UNKNOWN;
constexpr int UNKPAIR = (int)(((unsigned)(UNK & 0xffff) << 16) | (unsigned)(UNK & 0xffff));
constexpr int KNOWNPAIR = (int)(((unsigned)(LAYER_WINDOW_KNOWN & 0xffff) << 16) | (unsigned)(LAYER_WINDOW_KNOWN & 0xffff));

// Value of lane - 1 (lane 0 reads lane 63: wave_ror:1), `fill` in the lanes where `edge` is all ones.  The fill goes in through a
// v_bitop3, not a select: a select on the result of a DPP move is turned into a branch around the move, and the lanes the branch
// disables are then read by their neighbours (the hazard dpp_shr1 of rg_device.hpp describes; its empty asm was sunk into the
// branch with the move here).
__device__ __forceinline__ int left_lane(int v, int edge, int fill) {
    int r = __builtin_amdgcn_update_dpp(v, v, 0x13C, 0xf, 0xf, false);
    asm volatile("" : "+v"(r));
    return bfi(edge, fill, r);
}

}  // namespace

template <int C, int CW>
__global__ __launch_bounds__(64, 8) void k_layer_win(LayerArgs a) {
    static_assert(CW == 2 || CW == 4, "a column block is half a byte or a byte of the layer buffer");
    static_assert(C == 4 || C == 8 || C == 16, "packed rows, one direction word per lane and row");
    constexpr int H = CW / 2;
    constexpr int W = WAVE * CW;
    constexpr int WPAD = WAVE * C;
    constexpr int NBLK = WPAD / CW;
    constexpr unsigned LOWH = (1u << H) - 1u;
    constexpr unsigned FULL = (LOWH << 16) | LOWH;
    const int rd = blockIdx.x;
    const int lane = threadIdx.x;
    const PathGraphDev& g = a.g;
    LayerJob job;
    if (!job.open(a, rd, ST_BAD_BASE | ST_WOULD_PANIC | ST_OVERFLOW | ST_RETRY | ST_LAYER_FULL, false)) return;
    ReadState* rs = job.rs;
    const bool rev = a.rev;
    const int path = job.path, n = job.n, ncols = job.ncols;
    const uint8_t* read = job.read;
    const int GAP = 5;
    __shared__ int sct[64];              // [36]
    __shared__ int s2[5 * 64];           // packed (s - g) pairs by row base and (code_lo | code_hi << 3)
    __shared__ int kkp[NBLK];            // per column block: the code pairs of its registers (register r in byte r)
    if (lane < 36) sct[lane] = a.sc.t[lane];
    __syncthreads();
    const int gcost = __builtin_amdgcn_readfirstlane(sct[GAP]);
    pair_table(s2, sct, gcost, lane);
    auto code = [&](int c) -> int { return (c >= 1 && c < ncols) ? (int)(rev ? read[n - c + 1] : read[c]) : 4; };
    for (int b = lane; b < NBLK; b += WAVE) {
        int kk = 0;
#pragma unroll
        for (int r = 0; r < H; ++r) kk |= (code(b * CW + r) | (code(b * CW + H + r) << 3)) << (8 * r);
        kkp[b] = kk;
    }
    __syncthreads();
    // the walk's start cell (k_trace)
    const int start_col = job.start_col;
    const int sidx = __builtin_amdgcn_readfirstlane(layer_row_index(job.prow + job.pbase, job.nrows, job.start_row, rev));
    if (sidx < 0) return;                // (k_trace reports it)
    const int t_start = sidx + 1;
    uint8_t* tdir = reinterpret_cast<uint8_t*>(reinterpret_cast<uint32_t*>(a.layer) + (long long)rd * a.layer_stride);
    const uint32_t* dirs = a.dirs + (long long)rd * a.dirs_stride;
    // block of this lane in the window whose left edge is block lbk
    auto block_of = [&](int lbk) -> int { return lbk + ((lane - lbk) & (WAVE - 1)); };
    int lbk = layer_window_left(start_col, t_start, 0, W, WPAD) / CW;        // window of layer row 0: the gap-only start row, z = 0
    int blk = block_of(lbk);
    int kk = kkp[blk];
    int cur[H];
#pragma unroll
    for (int r = 0; r < H; ++r) {
        const int c0 = blk * CW + r, c1 = c0 + H;
        cur[r] = pack16(c0 < ncols ? 0 : UNK, c1 < ncols ? 0 : UNK);
    }
    // two-stage look-ahead as in k_layer16 (LayerJob::fetch_idx), over the rows up to the walk's start row
    constexpr int PF = 2;
    int pf_li[PF];
    uint32_t pf_w[PF];
    auto fetch_idx = [&](int tt) { job.fetch_idx(tt, sidx + 1); };
    auto prefetch = [&](int tt, int& li_o, uint32_t& w_o) {       // row tt, whose list entries are in nx_row / nx_slot
        li_o = 4; w_o = 0;
        if (job.nx_row >= 0) {
            const int b = block_of(layer_window_left(start_col, t_start, tt + 1, W, WPAD) / CW);
            li_o = g.lnz[job.nx_row];
            w_o = dirs[(long long)job.nx_slot * a.dir_words + (b * CW) / C];
        }
    };
#pragma unroll
    for (int k = 0; k < PF; ++k) { fetch_idx(k); prefetch(k, pf_li[k], pf_w[k]); }
    fetch_idx(PF);
    const int g_i = gcost;
    const int g0 = a.semi ? 0 : g_i;
    const int GI = pack16(g_i, g_i);
    for (int t = 0; t <= sidx; ++t) {
        const int li = pf_li[0];
        const uint32_t word = pf_w[0];
#pragma unroll
        for (int k = 0; k + 1 < PF; ++k) { pf_li[k] = pf_li[k + 1]; pf_w[k] = pf_w[k + 1]; }
        prefetch(t + PF, pf_li[PF - 1], pf_w[PF - 1]);
        fetch_idx(t + PF + 1);
        // ---- the window of this row: the lane whose block left takes the entering one ----
        const int nlbk = layer_window_left(start_col, t_start, t + 1, W, WPAD) / CW;
        if (nlbk != lbk) {
            lbk = nlbk;
            const int nb = block_of(lbk);
            const int nkk = kkp[nb];
            if (nb != blk) {
                kk = nkk;
#pragma unroll
                for (int r = 0; r < H; ++r) cur[r] = UNKPAIR;
            }
            blk = nb;
        }
        const int p = lbk & (WAVE - 1);                   // lane of the window's leftmost block
        const int pos = (lane - p) & (WAVE - 1);          // position of this lane's block in the window
        const int edge = pos == 0 ? -1 : 0;               // the window's left edge: the columns to the left are unknown
        const int GI0 = blk == 0 ? pack16(g0, g_i) : GI;  // border column 0 adds g0
        // direction bits of the lane's columns (bit q = column q of the sweep lane), then in register form (bit r: low half of
        // register r, bit 16 + r: high half)
        unsigned u16, l16;
        dir16_decode<C / 2>(word, u16, l16);
        const int q0 = (blk * CW) & (C - 1);
        const unsigned ub = u16 >> q0, lb = l16 >> q0;
        const unsigned um2 = (ub & LOWH) | (((ub >> H) & LOWH) << 16);
        const unsigned lm2 = (lb & LOWH) | (((lb >> H) & LOWH) << 16);
        int s[H], MU[H], ML[H];
#pragma unroll
        for (int r = 0; r < H; ++r) {
            s[r] = s2[li * 64 + ((kk >> (8 * r)) & 63)];
            MU[r] = pk_sub(0, (int)((um2 >> r) & (unsigned)ONE2));       // 0 - 1 = 0xffff per half
            ML[r] = pk_sub(0, (int)((lm2 >> r) & (unsigned)ONE2));
        }
        // nearest block to the left INSIDE the window that owns a non-L column (the ballot rotated by the window's phase)
        const unsigned long long have = __ballot(lm2 != FULL);
        const unsigned long long rot = p ? ((have >> p) | (have << (WAVE - p))) : have;
        const unsigned long long below = rot & ((1ull << pos) - 1ull);
        const int src = below ? ((63 - __clzll((long long)below) + p) & (WAVE - 1)) : -1;
        int old[H];
#pragma unroll
        for (int r = 0; r < H; ++r) old[r] = cur[r];
        // ---- the row update (RowOps16::member) ----
        int o1 = __builtin_amdgcn_alignbit(old[H - 1], left_lane(old[H - 1], edge, UNKPAIR), 16);        // old row, column c - 1
        {
            int prev = o1, lastv = UNKPAIR;
#pragma unroll
            for (int r = 0; r < H; ++r) {
                const int base = pk_add(bfi(MU[r], old[r], prev), bfi(MU[r], r == 0 ? GI0 : GI, s[r]));   // U: old + g_i, D: prev + (s - g)
                cur[r] = base;
                lastv = bfi(ML[r], lastv, base);
                prev = old[r];
            }
            const unsigned nl = ~lm2 & FULL;
            const int v_lo = lo16(lastv), v_hi = hi16(lastv);
            const int zl = (nl >> 16) ? v_hi : ((nl & 0xffffu) ? v_lo : UNK);
            const int fetched = __shfl(zl, src < 0 ? lane : src, WAVE);
            const int bl = src < 0 ? UNK : max(fetched, UNK);
            const int bh = (nl & 0xffffu) ? max(v_lo, UNK) : bl;
            int vprev = pack16(bl, bh);
#pragma unroll
            for (int r = 0; r < H; ++r) {
                int v = bfi(ML[r], vprev, cur[r]);
                v = bfi(pk_sign(pk_sub_sat(v, KNOWNPAIR)), UNKPAIR, v);    // unknown stays AT the sentinel
                cur[r] = v;
                vprev = v;
            }
        }
        // ---- traceback decisions of this row (k_layer16) ----
        const bool zero_prev = rev && t == 0 && path != 0;
        if (zero_prev) {
#pragma unroll
            for (int r = 0; r < H; ++r) {
                const int c0 = blk * CW + r, c1 = c0 + H;
                old[r] = pack16(-c0 * gcost, -c1 * gcost);
            }
            o1 = __builtin_amdgcn_alignbit(old[H - 1], left_lane(old[H - 1], edge, UNKPAIR), 16);
            if (blk == 0) o1 = pack16(gcost, hi16(o1));
        }
        int nl = __builtin_amdgcn_alignbit(cur[H - 1], left_lane(cur[H - 1], edge, UNKPAIR), 16);      // new row, column c - 1
        unsigned tw = 0;
#pragma unroll
        for (int r = 0; r < H; ++r) {
            const int d = pk_add(o1, s[r]);
            const int u = pk_add(old[r], GI);
            const int unk = pk_sign(pk_sub_sat(pk_min(pk_min(d, u), nl), KNOWNPAIR));     // 0xffff where an input is unknown
            const unsigned code2 = decide16(d, u, nl) & ~(unsigned)unk;
            tw |= code2 << (2 * r);
            o1 = old[r];
            nl = cur[r];
        }
        // codes of columns 0 .. H-1 of the block at bits 2r, of H .. CW-1 at bits 16 + 2r -> column order
        const unsigned codes = (tw & ((1u << (2 * H)) - 1u)) | ((tw >> 16) << (2 * H));
        const int c0 = blk * CW;
        uint8_t* out = tdir + (long long)(t + 1) * a.dir_words * 4 + ((c0 / C) * 4 + ((c0 & (C - 1)) >> 2));
        if constexpr (CW == 4) {
            *out = (uint8_t)codes;
        } else {
            // two blocks share a byte: the even one (its partner is the next lane, inside the window: the left edge is a multiple of 4 columns) stores it
            const unsigned other = (unsigned)__builtin_amdgcn_update_dpp(0, (int)codes, 0xF5, 0xf, 0xf, false);   // quad_perm [1, 1, 3, 3]
            if (!(lane & 1)) *out = (uint8_t)(codes | (other << 4));
        }
        if (t == sidx && !rev) {
            // the value at the start cell; when the window does not hold it the full-width kernels take the read
            const int q = start_col & (CW - 1);
            int pv = 0;
#pragma unroll
            for (int r = 0; r < H; ++r) if (r == q % H) pv = cur[r];
            const int z = q >= H ? hi16(pv) : lo16(pv);
            if (blk == start_col / CW) {
                if (z < LAYER_WINDOW_KNOWN) atomicOr(&rs->status, ST_LAYER_FULL);
                else rs->trace_score = z + start_col * gcost;
            }
        }
    }
}

const char* launch_layer_window(const LayerArgs& a, int nreads, int C, int window, hipStream_t s) {
    if (window == LAYER_WINDOW_NARROW) RG_SWITCH_C((4, 8, 16), k_layer_win, (, 2), dim3(nreads), dim3(64), 0, s, a);
    RG_SWITCH_C((4, 8, 16), k_layer_win, (, 4), dim3(nreads), dim3(64), 0, s, a);
}

}  // namespace rg
