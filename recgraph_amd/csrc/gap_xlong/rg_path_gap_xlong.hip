// Affine-gap pathwise alignment of very long reads for gfx950 (-m 56 global, -m 57 semiglobal, -m 62 local): the rules of -m 6, -m 7 and
// -m 12 for reads of up to 131071 bases (64 column stripes of 2048).  Score pass and pick are the kernels of -m 16 / -m 17 / -m 22
// (k_gap_score_long, k_gap_pick, k_gap_pick_local); what is new is the traceback, which keeps the direction words of ONE stripe:
//
//   k_gap_ckpt_long<kind>   one wave per read: the row step of k_gap_dirs_long for the picked path WITHOUT direction words; what each
//                           stripe leaves to its right neighbour stays, per row, in a checkpoint slot of its own.  Sets up the walk.
//   then, for round r = S - 1 down to 0, with no read-back in between:
//   k_gap_redo_long<kind>   one wave per read whose walk stands in stripe r: the row step again, from checkpoint slot r - 1, rows 1 to
//                           the walk's row only, 4 bits per cell into the one-stripe buffer (the layout of one stripe of k_gap_dirs_long)
//   k_gap_walk_long, k_gap_walk_local_long   the walks of k_gap_trace_long / k_gap_trace_local_long, resumed from the saved state; a
//                           round ends when the column leaves stripe r on the left (the state is saved) or when the walk is done (the
//                           record is written as those kernels write it)
//
// A walk only ever moves left and up, so it enters every stripe at most once, in descending order, and never needs a row below the
// one it entered with.  In round r an unfinished walk stands in a stripe <= r: it starts in a stripe <= S - 1 and leaves round r in
// a stripe < r.  A stripe above the round is an inconsistent state and ends as ST_WOULD_PANIC; round 0 finishes every walk.  The
// rebuild and the walk are separate launches: the walk reads what another kernel wrote.
//
// The row step, the nibble lookup, the walk and the record writer are the family's (gap/rg_path_gap_common.hpp: gap_row, dir_cell,
// gap_walk), the stripe geometry and the boundary exchange those of gap_long/ (rg_path_gap_long_rows.hpp): the same registers hold
// the same values, so a rebuilt word equals the word k_gap_dirs_long stores for that (stripe, row, lane).
#include <type_traits>

#include "rg_path_gap_xlong.hpp"

namespace rg {

namespace {

#include "../gap/rg_path_gap_common.hpp"
#include "../gap_long/rg_path_gap_long_rows.hpp"    // CL, STRIPE, WL, Boundary

// checkpoint slot s of a read: [2][rows1]
__device__ __forceinline__ int* ckpt_slot(const GapXLongArgs& xa, int rd, int s) {
    return xa.ckpt + (long long)rd * xa.ckpt_stride + 2ll * s * xa.l.rows1;
}

}  // namespace

template <int kKind>
__global__ __launch_bounds__(64) void k_gap_ckpt_long(GapXLongArgs xa) {
    constexpr bool kLocal = kKind == GAP_LOCAL;
    __shared__ int sct[40];
    const GapLongArgs& la = xa.l;
    const GapArgs& a = la.g;
    const int rd = blockIdx.x, lane = threadIdx.x;
    ReadState* rs = a.state + rd;
    if (rs->status & ST_NO_RECORD) return;
    const long long ro = a.read_off[rd];
    const int n = __builtin_amdgcn_readfirstlane((int)(a.read_off[rd + 1] - ro));
    const int k = __builtin_amdgcn_readfirstlane(rs->fwd_path);
    const int score = __builtin_amdgcn_readfirstlane(rs->trace_score);
    const int pbeg = a.poff[k];
    int m = a.poff[k + 1] - pbeg;
    const int idx = __builtin_amdgcn_readfirstlane(row_index(a.prow + pbeg, m, rs->end_row));      // where the walk starts
    if (kKind != GAP_GLOBAL) m = idx + 1;        // the rows up to the end row are all the walk can visit
    m = __builtin_amdgcn_readfirstlane(min(m, la.rows1 - 1));
    if (n + 1 > la.S * STRIPE || idx < 0 || idx + 1 >= la.rows1 || (kLocal && m <= 0)) {
        if (lane == 0) rs->status = ST_WOULD_PANIC;
        return;
    }
    load_scores(a, lane, sct);
    const int S = (n + STRIPE) / STRIPE;
    Boundary bd;
    NoDirs nd;
    int end_col = 0;                                 // local: the smallest global column of the end row that holds the score (0: none yet)
    for (int s = 0; s < S; ++s) {
        const int c0 = s * STRIPE;
        const bool first = s == 0, last = s == S - 1;
        int* const from = ckpt_slot(xa, rd, first ? 0 : s - 1);      // (stripe 0 reads nothing, the last stripe writes nothing)
        int* const to = ckpt_slot(xa, rd, last ? 0 : s);
        int H[CL], Y[CL];
        ReadCols<CL, false> rc;
        rc.load(a.reads + ro - 1, n, lane, c0);
        row0<CL, kKind>(H, Y, a.o, a.e, c0, lane);
        const int ej0 = a.e * (c0 + lane * CL);
        bd.begin_stripe(first, kLocal ? 0 : a.o + a.e * (c0 - 1));      // H[0][c0 - 1]
        int c = CL;
        for (int t0 = 0; t0 < m; t0 += WAVE) {
            int myb = 4;
            if (t0 + lane < m) myb = a.lnz[a.prow[pbeg + t0 + lane]];
            bd.h = from; bd.z = from + la.rows1;
            bd.begin_block(first, t0, m, lane);
            const int cnt = min(WAVE, m - t0);
            for (int u = 0; u < cnt; ++u) {
                const int b = __builtin_amdgcn_readlane(myb, u);
                const int incl = gap_row<CL, kKind, true>(H, Y, rc, sct, b, a.o, a.e, ej0, lane == 0, first && lane == 0, bd.dnext, bd.zin(u), nd);
                bd.after_row(u, lane, H[CL - 1], incl);
                if (kLocal && t0 + u == m - 1) c = own_end_col(H, score, c);      // H is the end row (as in k_gap_dirs_long<2>)
            }
            bd.h = to; bd.z = to + la.rows1;
            bd.end_block(last, t0, m, lane);
        }
        // stripes in ascending order: the first one that holds the score decides
        if (kLocal && end_col == 0) end_col = wave_end_col<CL>(c, c0);
    }
    if (lane == 0) {
        if (kLocal && (end_col < 1 || end_col > n)) {
            rs->status = ST_WOULD_PANIC;              // the score pass and this one disagree: never a guess
        } else {
            if (kLocal) rs->rec_col = end_col;
            GapWalkState* ws = xa.walk + rd;
            ws->i = idx + 1; ws->j = kLocal ? end_col : n; ws->state = S_H;
            ws->nops = 0; ws->steps = 0; ws->done = 0;
        }
        if (m > 0) atomicAdd(a.cells + 1, (unsigned long long)m * (unsigned long long)n);
    }
}

template <int kKind>
__global__ __launch_bounds__(64) void k_gap_redo_long(GapXLongArgs xa, int round) {
    constexpr bool kLocal = kKind == GAP_LOCAL;
    __shared__ int sct[40];
    const GapLongArgs& la = xa.l;
    const GapArgs& a = la.g;
    const int rd = blockIdx.x, lane = threadIdx.x;
    const ReadState* rs = a.state + rd;
    if (rs->status & ST_NO_RECORD) return;
    const GapWalkState* ws = xa.walk + rd;
    if (ws->done) return;
    const int wi = __builtin_amdgcn_readfirstlane(ws->i), wj = __builtin_amdgcn_readfirstlane(ws->j);
    if (wi <= 0 || wj <= 0 || wj / STRIPE != round) return;      // the walk is not in this stripe (a stripe above the round: the walk kernel reports it)
    const long long ro = a.read_off[rd];
    const int n = __builtin_amdgcn_readfirstlane((int)(a.read_off[rd + 1] - ro));
    const int k = __builtin_amdgcn_readfirstlane(rs->fwd_path);
    const int pbeg = a.poff[k];
    const int m = __builtin_amdgcn_readfirstlane(min(min(wi, a.poff[k + 1] - pbeg), la.rows1 - 1));      // rows 1 .. the walk's row
    if (wj > n || n + 1 > la.S * STRIPE) return;                 // (the walk kernel reports it)
    load_scores(a, lane, sct);
    const int c0 = round * STRIPE;
    const bool first = round == 0;
    int* const from = ckpt_slot(xa, rd, first ? 0 : round - 1);
    Boundary bd;
    bd.h = from; bd.z = from + la.rows1;
    uint32_t* sout = a.dirs + (long long)rd * a.dirs_stride;
    DirWords<CL> dw;
    int H[CL], Y[CL];
    ReadCols<CL, true> rc;
    rc.load(a.reads + ro - 1, n, lane, c0);
    row0<CL, kKind>(H, Y, a.o, a.e, c0, lane);
    const int ej0 = a.e * (c0 + lane * CL);
    bd.begin_stripe(first, kLocal ? 0 : a.o + a.e * (c0 - 1));      // H[0][c0 - 1]
    for (int t0 = 0; t0 < m; t0 += WAVE) {
        int myb = 4;
        if (t0 + lane < m) myb = a.lnz[a.prow[pbeg + t0 + lane]];
        bd.begin_block(first, t0, m, lane);
        const int cnt = min(WAVE, m - t0);
        for (int u = 0; u < cnt; ++u) {
            const int b = __builtin_amdgcn_readlane(myb, u);
            const int incl = gap_row<CL, kKind, true>(H, Y, rc, sct, b, a.o, a.e, ej0, lane == 0, first && lane == 0, bd.dnext, bd.zin(u), dw);
            bd.after_row(u, lane, H[CL - 1], incl);
#pragma unroll
            for (int w = 0; w < WL; ++w) sout[((long long)(t0 + u + 1) * WL + w) * WAVE + lane] = dw.w[w];
        }
        // (nothing to leave: the stripe to the right is done with)
    }
    if (lane == 0 && m > 0) {
        const int cols = min(n, c0 + STRIPE - 1) - max(1, c0) + 1;      // the stripe's columns that belong to the read
        atomicAdd(a.cells + 1, (unsigned long long)m * (unsigned long long)cols);
    }
}

namespace {

// One round of a walk: gap_walk resumed from the saved state, over the one-stripe buffer that holds stripe `round`.  The iteration
// count runs over all rounds.
template <bool kLocal>
__device__ __forceinline__ void walk_round(const GapXLongArgs& xa, int semi, int round) {
    const GapLongArgs& la = xa.l;
    const GapArgs& a = la.g;
    const int rd = blockIdx.x, lane = threadIdx.x;
    const ReadState* rs = a.state + rd;
    DevRecord* rec = a.rec + rd;
    GapWalkState* ws = xa.walk + rd;
    auto over = [&] { if (lane == 0) ws->done = 1; };      // the record, or its absence, is written
    if (rs->status & ST_NO_RECORD) {
        if (round == la.S - 1) { no_record(rec, lane, rs->status); over(); }      // (no walk state: reported in the first round)
        return;
    }
    if (ws->done) return;
    const int n = (int)(a.read_off[rd + 1] - a.read_off[rd]);
    const int k = rs->fwd_path;
    const int m = a.poff[k + 1] - a.poff[k];
    WalkPos p{ws->i, ws->j, ws->state, ws->nops, ws->steps};
    // an unfinished walk stands on a cell inside the matrix, in a stripe at or below the round
    if (p.i < 1 || p.i > m || p.i >= la.rows1 || p.j < 1 || p.j > n || n + 1 > la.S * STRIPE || (unsigned)p.state > (unsigned)S_XARRIVE ||
        p.nops < 0 || p.steps < 0 || p.j / STRIPE > round) {
        no_record(rec, lane, ST_WOULD_PANIC);
        over();
        return;
    }
    if (p.j / STRIPE < round) return;                // its stripe comes in a later round
    if (gap_walk<kLocal>(a, rd, lane, semi, kLocal ? rs->rec_col : n, p, round * STRIPE, CL, la.rows1)) over();
    else if (lane == 0) { ws->i = p.i; ws->j = p.j; ws->state = p.state; ws->nops = p.nops; ws->steps = p.steps; }      // the next stripe's round goes on from here
}

}  // namespace

// The walk of -m 6 / -m 7 (k_gap_trace_long), one stripe per launch.
__global__ __launch_bounds__(64) void k_gap_walk_long(GapXLongArgs xa, int semi, int round) { walk_round<false>(xa, semi, round); }

// The walk of -m 12 (k_gap_trace_local_long), one stripe per launch: from (end row, end column) until a cell with H == 0.
__global__ __launch_bounds__(64) void k_gap_walk_local_long(GapXLongArgs xa, int round) { walk_round<true>(xa, 0, round); }

// ---- launchers ---------------------------------------------------------------------------------------------------------------
static bool geometry_ok(const GapXLongArgs& a) {
    return a.l.S >= 2 && a.l.S <= GAP_XLONG_MAX_STRIPES && a.l.rows1 >= 1 && a.l.g.dirs && a.l.g.dirs_stride >= (long long)a.l.rows1 * WL * WAVE &&
           a.ckpt && a.ckpt_stride >= 2ll * (a.l.S - 1) * a.l.rows1 && a.walk;
}

const char* launch_gap_ckpt_long(const GapXLongArgs& a, int nreads, int kind, hipStream_t s) {
    if (!geometry_ok(a)) return nullptr;
    const dim3 grid(nreads);
    RG_GAP_SWITCH_KIND(k_gap_ckpt_long, grid, a);
    return nullptr;
}
const char* launch_gap_redo_long(const GapXLongArgs& a, int nreads, int kind, int round, hipStream_t s) {
    if (!geometry_ok(a) || round < 0 || round >= a.l.S) return nullptr;
    const dim3 grid(nreads);
    RG_GAP_SWITCH_KIND(k_gap_redo_long, grid, a, round);
    return nullptr;
}
const char* launch_gap_walk_long(const GapXLongArgs& a, int nreads, int kind, int round, hipStream_t s) {
    if (!geometry_ok(a) || round < 0 || round >= a.l.S) return nullptr;
    if (kind == GAP_LOCAL) RG_LAUNCH0(k_gap_walk_local_long, dim3(nreads), dim3(WAVE), 0, s, a, round);
    if (kind != GAP_GLOBAL && kind != GAP_SEMI) return nullptr;
    RG_LAUNCH0(k_gap_walk_long, dim3(nreads), dim3(WAVE), 0, s, a, kind == GAP_SEMI ? 1 : 0, round);
}

}  // namespace rg
