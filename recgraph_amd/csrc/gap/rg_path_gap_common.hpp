// What the kernel files of the affine-gap pathwise family share (gap/: -m 6 / -m 7; gap_local/: -m 12; gap_long/: -m 16 / -m 17 /
// -m 22; gap_xlong/: -m 56 / -m 57 / -m 62): the ONE row step of the rule and what surrounds it (sentinel, direction words, base
// codes, row 0, score table, column pick), the bodies of the single-wave score, pick and trace kernels, the ONE walk of
// the direction nibbles with its record writer, and the two dispatch macros of the launchers.  The `__global__` functions of the
// four files are callers of these.  Everything here is inlined into its callers; included inside namespace rg, in each file's
// anonymous namespace, after gap/rg_path_gap.hpp (GapArgs, GapKind).
#pragma once

constexpr int GNEG = -(1 << 29);
constexpr int gap_words(int C) { return C >= 8 ? C / 8 : 1; }

// The base codes of the lane's columns, in the stripe that starts at global column c0 (4 = N for column 0 and the columns past the
// read).  kPack: four codes per dword — the direction pass, whose masks and packed words compete with the three C-wide arrays for
// registers, pays one v_bfe per cell for 3 C / 4 registers
template <int C, bool kPack>
struct ReadCols {
    int v[kPack ? C / 4 : C];
    __device__ __forceinline__ void load(const uint8_t* read /* read[1..n] */, int n, int lane, int c0 = 0) {
#pragma unroll
        for (int i = 0; i < (kPack ? C / 4 : C); ++i) v[i] = 0;
#pragma unroll
        for (int q = 0; q < C; ++q) {
            const int j = c0 + lane * C + q;
            const int code = (j >= 1 && j <= n) ? (int)read[j] : 4;
            if (kPack) v[q / 4] |= code << (8 * (q % 4));
            else v[q] = code;
        }
    }
    __device__ __forceinline__ int get(int q) const { return kPack ? (v[kPack ? q / 4 : 0] >> (8 * (q % 4))) & 0xff : v[kPack ? 0 : q]; }
};

// the direction words of one row (the direction passes) / nothing (the score passes: the row step then has no direction code at all)
template <int C>
struct DirWords { uint32_t w[gap_words(C)]; };
struct NoDirs {};

// index of `row` among the ascending rows of a path (-1: not there)
__device__ __forceinline__ int row_index(const int* rows, int m, int row) {
    int lo = 0, hi = m - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1, r = rows[mid];
        if (r == row) return mid;
        if (r < row) lo = mid + 1; else hi = mid - 1;
    }
    return -1;
}

// the score table in LDS as [path base][8]
__device__ __forceinline__ void load_scores(const GapArgs& a, int lane, int* sct) {
    if (lane < 40) { const int b = lane >> 3, c = lane & 7; sct[lane] = c < 5 ? a.sc.t[b * 6 + c] : 0; }
    __syncthreads();
}

// row 0 of the stripe that starts at column c0: H = X = o + e j (0 at column 0; 0 everywhere in the local kind), Y = NEG
template <int C, int kKind>
__device__ __forceinline__ void row0(int (&H)[C], int (&Y)[C], int o, int e, int c0, int lane) {
#pragma unroll
    for (int q = 0; q < C; ++q) {
        const int j = c0 + lane * C + q;
        H[q] = (kKind == GAP_LOCAL || j == 0) ? 0 : o + e * j;
        Y[q] = GNEG;
    }
}

// THE ROW STEP (derived in gap/rg_path_gap.hip): one path row with base b.  kKind: global has no column-0 rule (the recurrence
// itself gives o + e i); semi and local hold H[i][0] = 0, Y[i][0] = NEG where col0 says that the lane's first column is column 0 of
// the read; local clamps H' at 0, and the scan stays exact with the clamped H' by the same argument (o <= 0).
// kStriped (gap_long/, gap_xlong/): din is H[i-1][c0-1], lane 0's diagonal; zin the row's z maximum over the stripes to the left
// (both NEG in stripe 0).  Returns the inclusive z maximum up to and including this lane (striped: zin included, so lane 63 holds
// what the next stripe needs).  An unstriped caller compiles to the data flow without din and zin: no select, no max.
// Dirs = DirWords<C>: 4 bits per cell: bits 0-1 the source of H (1 D, 2 U, 3 L; local: 0 = "H == 0: the walk stops here"), bit 2
// "Y[i][j] was opened from H[i-1][j]", bit 3 "an X run that goes on to column j + 1 opens here" (H[i][j] + o >= X[i][j]).
template <int C, int kKind, bool kStriped, class Dirs, class Cols>
__device__ __forceinline__ int gap_row(int (&H)[C], int (&Y)[C], const Cols& rc, const int* sct, int b, int o, int e, int ej0, bool lane0, bool col0,
                                       int din, int zin, Dirs& dw) {
    constexpr bool kDirs = !std::is_same_v<Dirs, NoDirs>;
    constexpr bool kLocal = kKind == GAP_LOCAL;
    // The nibble as selects in the single-wave global and semi passes: on an MI355X the sign-bit form with the pin costs k_gap_dirs
    // 14 - 34 % (13 - 29 % more instructions), and one wave per read has no use for the occupancy it buys (profiles/gap_family_notes.md).
    // The local kind's third select (the stop code) and the stripe inputs do not fit that way: 238 and 246 registers at C = 32
    constexpr bool kSelects = !kLocal && !kStriped;
    const int* srow = sct + b * 8;
    const int oe = o + e;
    int diag = dpp_shr1(H[C - 1], GNEG);           // lane 0: column 0 has no diagonal
    if constexpr (kStriped) diag = lane0 ? din : diag;
    unsigned dm = 0, ym = 0;
    int acc = GNEG;                                // max_q (H'_q + e (C - 1 - q)): the lane's z maximum, taken at its last column
#pragma unroll
    for (int q = 0; q < C; ++q) {
        const int hold = H[q], yold = Y[q];
        int y = max(hold + oe, yold + e);
        const int d = diag + srow[rc.get(q)];
        int hp = max(d, y);
        if (kLocal) hp = max(hp, 0);
        if (kKind != GAP_GLOBAL && q == 0) {
            hp = col0 ? 0 : hp;
            y = col0 ? GNEG : y;
        }
        if constexpr (kDirs && kSelects) {
            dm |= (d >= y ? 1u : 0u) << q;
            ym |= (hold + o >= yold ? 1u : 0u) << q;
        } else if constexpr (kDirs) {
            // d >= y and hold + o >= yold as sign bits (every difference lies inside +-2^31): a select of the constant 1 << q per
            // column kept two dozen registers of constants
            dm |= ((unsigned)(y - d - 1) >> 31) << q;
            ym |= ((unsigned)(yold - (hold + o) - 1) >> 31) << q;
        }
        diag = hold;
        Y[q] = y;
        H[q] = hp;
        acc = max(acc + e, hp);
    }
    // striped: the masks stay where they are computed: sunk to their use, d, y, hold, yold of every column stay live (the first
    // build of k_gap_dirs_long took 246 registers).  The single-wave passes fit without the pin, and it costs them 3 - 21 % on an
    // MI355X: it makes the masks early
    if constexpr (kDirs && kStriped) asm volatile("" : "+v"(dm), "+v"(ym));
    // z of the lane = acc - e (lane C + C - 1); the exclusive maximum over the lanes to the left gives X of the lane's first column,
    // and inside the lane X runs on as X_{j+1} = max(X_j, H'_j + o) + e — the same values as run + o + e j without a z or an e j per
    // column held in registers across the rows
    int incl = dpp_incl_max(acc - (ej0 + e * (C - 1)), GNEG);
    if constexpr (kStriped) incl = max(incl, zin);
    int zl = dpp_shr1(incl, GNEG);
    if constexpr (kStriped) zl = max(zl, zin);
    int x = zl + o + ej0;
    if constexpr (kDirs) {
#pragma unroll
        for (int w = 0; w < gap_words(C); ++w) dw.w[w] = 0;
    }
#pragma unroll
    for (int q = 0; q < C; ++q) {
        const int hp = H[q];
        const int h = max(hp, x);
        if constexpr (kDirs && kSelects) {
            const unsigned src = hp >= x ? (((dm >> q) & 1u) ? 1u : 2u) : 3u;
            const unsigned nib = src | (((ym >> q) & 1u) << 2) | ((h + o >= x ? 1u : 0u) << 3);
            dw.w[q / 8] |= nib << (4 * (q % 8));
        } else if constexpr (kDirs) {
            const unsigned t = (unsigned)(x - hp - 1) >> 31;                  // hp >= x
            // L 3; else D 1 if d >= y, U 2 otherwise.  As arithmetic on sign bits: as selects (with the constants 1 << q of the masks
            // above) k_gap_dirs_local<32> took 238 registers
            unsigned src = 3u - t - (t & (dm >> q));
            if (kLocal) src &= (unsigned)(-h >> 31);                          // 0 where h == 0 (h >= 0)
            const unsigned nib = src | (((ym >> q) & 1u) << 2) | (((unsigned)(x - (h + o) - 1) >> 31) << 3);     // h + o >= x
            dw.w[q / 8] |= nib << (4 * (q % 8));
        }
        H[q] = h;
        x = max(x, hp + o) + e;
    }
    return incl;
}

// value of column qn (wave-uniform) of the lane's chunk.  As a maximum over selects with a constant arm: a chain of
// `q == qn ? H[q] : v` is turned into a dynamically indexed array by the compiler, which then moves H out of the registers
template <int C>
__device__ __forceinline__ int pick_col(const int (&H)[C], int qn) {
    int v = INT32_MIN;
#pragma unroll
    for (int q = 0; q < C; ++q) v = max(v, q == qn ? H[q] : INT32_MIN);
    return v;
}

// Local kind: the best of the lane's own columns 0 .. qlim, the ones that belong to the read (none: qlim negative; column 0 is
// H = 0 and never beats the initial 0).  Columns past the read (base code N) depend only on cells to their left, so they cannot
// disturb real cells — but they CAN hold positive values (X running on, or a matrix whose N entries are positive), so they never
// compete: every lane compares against its limit qlim = min(C - 1, n - first column of the lane)
template <int C>
__device__ __forceinline__ int best_own_col(const int (&H)[C], int qlim) {
    int v = 0;
#pragma unroll
    for (int q = 0; q < C; ++q) v = max(v, q <= qlim ? H[q] : 0);
    return v;
}

// Local kind, at the end row: the lane's smallest column that holds the score (c: the value so far, C = none), and over the wave the
// smallest global column (lowest lane, then lowest column of that lane; 0: none).  No test against the read's end: the score pass
// found such a column inside the read, so the smallest one is inside it too (the callers check).  The callers run own_end_col INSIDE
// the row loop: behind it, H live out of the loop cost k_gap_dirs_local<32> 10 registers
template <int C>
__device__ __forceinline__ int own_end_col(const int (&H)[C], int score, int c) {
#pragma unroll
    for (int q = C - 1; q >= 0; --q) c = H[q] == score ? q : c;
    return c;
}
template <int C>
__device__ __forceinline__ int wave_end_col(int c, int c0) {
    const unsigned long long hit = __ballot(c < C);
    if (!hit) return 0;
    const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)hit) - 1);
    return c0 + l * C + __builtin_amdgcn_readlane(c, l);
}

// ---- the single-wave passes: lane t owns the C consecutive columns t * C .. t * C + C - 1 of the (n + 1)-column row ----------------

// one wave per (read, path) -> ReadState::sink_val (global: the last-column value of the path; semi: its best over the rows; local:
// the best H over rows >= 1 and the read's columns) and, semi and local, path_end_row: the first row that attains it
template <int C, int kKind>
__device__ __forceinline__ void gap_score_wave(const GapArgs& a, int* sct) {
    constexpr bool kLocal = kKind == GAP_LOCAL;
    const int rd = blockIdx.y, k = blockIdx.x, lane = threadIdx.x;
    const long long ro = a.read_off[rd];
    const int n = __builtin_amdgcn_readfirstlane((int)(a.read_off[rd + 1] - ro));
    if (a.bad[rd] || n + 1 > C * WAVE) return;     // (the pick kernel reports the read)
    const int pbeg = a.poff[k], m = a.poff[k + 1] - pbeg;
    int H[C], Y[C];
    ReadCols<C, false> rc;
    rc.load(a.reads + ro - 1, n, lane);
    load_scores(a, lane, sct);
    row0<C, kKind>(H, Y, a.o, a.e, 0, lane);
    const int ln = n / C, qn = n % C, ej0 = a.e * lane * C, qlim = min(C - 1, n - lane * C);
    int best = kLocal ? 0 : GNEG, bt = 0;          // (local: per lane, over its own columns)
    NoDirs nd;
    // the bases of 64 path rows per gather (two dependent loads per row would cost more than the row step)
    for (int t0 = 0; t0 < m; t0 += WAVE) {
        int myb = 4;
        if (t0 + lane < m) myb = a.lnz[a.prow[pbeg + t0 + lane]];
        const int cnt = min(WAVE, m - t0);
        for (int u = 0; u < cnt; ++u) {
            const int b = __builtin_amdgcn_readlane(myb, u);
            gap_row<C, kKind, false>(H, Y, rc, sct, b, a.o, a.e, ej0, lane == 0, lane == 0, GNEG, GNEG, nd);
            if (kKind != GAP_GLOBAL) {
                const int v = kLocal ? best_own_col<C>(H, qlim) : pick_col<C>(H, qn);
                if (v > best) { best = v; bt = t0 + u; }      // strictly better: the first row that attains the maximum
            }
        }
    }
    if (kLocal) {
        // the one cross-lane step: highest value, then the smallest row
#pragma unroll
        for (int d = WAVE / 2; d >= 1; d >>= 1) {
            const int v = __shfl_xor(best, d, WAVE), t = __shfl_xor(bt, d, WAVE);
            if (v > best || (v == best && t < bt)) { best = v; bt = t; }
        }
    }
    if (lane == (kLocal ? 0 : ln)) {
        ReadState* rs = a.state + rd;
        rs->sink_val[k] = kKind == GAP_GLOBAL ? pick_col<C>(H, qn) : best;
        if (kKind != GAP_GLOBAL) rs->path_end_row[k] = m > 0 ? a.prow[pbeg + bt] : 0;
    }
    if (lane == 0) {
        const unsigned long long c = (unsigned long long)m * (unsigned long long)n;
        atomicAdd(a.cells, c);
        atomicAdd(a.cells + 1, c);
    }
}

// One wave per read: (score, end row, path) of the read.  Global: highest score, then lowest path; semi and local: highest score,
// then smallest row, then lowest path.  Local: a best value of 0 is "no local alignment": ST_UNALIGNED
template <bool kLocal>
__device__ __forceinline__ void gap_pick_wave(const GapArgs& a, int wcols, int semi) {
    const int rd = blockIdx.x, lane = threadIdx.x;
    ReadState* rs = a.state + rd;
    const int n = (int)(a.read_off[rd + 1] - a.read_off[rd]);
    if (a.bad[rd] || n + 1 > wcols) {
        if (lane == 0) rs->status = a.bad[rd] ? ST_BAD_BASE : ST_WOULD_PANIC;
        return;
    }
    const bool rows = kLocal || semi;              // the score pass left an end row per path
    int bv = INT32_MIN, br = INT32_MAX, bk = INT32_MAX;
    auto better = [](int v, int r, int k, int v2, int r2, int k2) { return v != v2 ? v > v2 : r != r2 ? r < r2 : k < k2; };
    for (int k = lane; k < a.P; k += WAVE) {
        const int v = rs->sink_val[k], r = rows ? rs->path_end_row[k] : 0;
        if (better(v, r, k, bv, br, bk)) { bv = v; br = r; bk = k; }
    }
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) {
        const int v = __shfl_xor(bv, d, WAVE), r = __shfl_xor(br, d, WAVE), k = __shfl_xor(bk, d, WAVE);
        if (better(v, r, k, bv, br, bk)) { bv = v; br = r; bk = k; }
    }
    if (lane == 0) {
        if (kLocal && (bv <= 0 || bk < 0 || bk >= a.P)) { rs->status = bv == 0 ? ST_UNALIGNED : ST_WOULD_PANIC; return; }
        const int end = rows ? br : a.prow[a.poff[bk + 1] - 1];
        rs->s0 = bv; rs->bound = bv; rs->trace_score = bv;
        rs->seed_path = bk; rs->fwd_path = bk; rs->rev_path = bk;
        rs->end_row = end; rs->end_row_best = end;
    }
}

// ---- the walk --------------------------------------------------------------------------------------------------------------------

// The direction nibble of cell (i, j) of the picked path, j counted from the buffer's first column.  Stripe s = j / (64 C) of row i
// lies at ((s * rows1 + i) * W + w) * 64 + lane; a single-wave buffer is stripe 0 alone.  The row's words of one stripe are cached per
// (row, stripe) in `have`.  C is a power of two (4, 8, 16, 32: the launchers admit nothing else) and cs its logarithm, so the cell's
// place is shifts and masks: no division by a run-time C, and the constants of old where the caller knows C at compile time
__device__ __forceinline__ uint32_t dir_cell(const uint32_t* dirs, int C, int cs, int rows1, int lane, int i, int j, int& have, uint32_t (&wd)[4]) {
    const int W = gap_words(C), s = j >> (cs + 6), jl = j & (C * WAVE - 1);
    const int key = s * rows1 + i;
    if (have != key) {
#pragma unroll
        for (int w = 0; w < 4; ++w)
            if (w < W) wd[w] = dirs[((long long)key * W + w) * WAVE + lane];
        have = key;
    }
    const int q = jl & (C - 1), wsel = q >> 3;
    const uint32_t word = wsel == 0 ? wd[0] : wsel == 1 ? wd[1] : wsel == 2 ? wd[2] : wd[3];
    return ((uint32_t)__builtin_amdgcn_readlane((int)word, __builtin_amdgcn_readfirstlane(jl >> cs)) >> (4 * (q & 7))) & 15u;
}

__device__ __forceinline__ void no_record(DevRecord* rec, int lane, uint32_t st) {
    if (lane == 0) { rec->status = st; rec->n_ops = 0; rec->n_fwd_ops = 0; rec->score = 0; }
}

__device__ __forceinline__ void write_record(DevRecord* rec, int lane, const ReadState* rs, int end_col, int stop_row, int stop_col, int nops) {
    if (lane == 0) {
        rec->status = rs->status;
        rec->score = rs->trace_score;
        rec->fscore = 0.f;
        rec->end_row = rs->end_row;
        rec->end_col = end_col;
        rec->stop_row = stop_row; rec->stop_col = stop_col;
        rec->best_path = rs->fwd_path; rec->rev_path = rs->fwd_path;
        rec->fen = 0; rec->rsn = 0; rec->rec_col = 0; rec->displacement = 0;
        rec->n_ops = nops; rec->n_fwd_ops = nops;
        rec->pad = 0;
    }
}

enum { S_H, S_Y, S_X, S_XARRIVE };
struct WalkPos { int i, j, state, nops, steps; };      // the cell the walk looks at next (row index + 1 of the picked path, read column)

// The walk of the rule from p over the direction words of the columns c0 and up (c0: the buffer's first column and the walk's lower
// column bound), to its end or until the column leaves the buffer on the left.  Returns true when the walk is over — the record is
// written, or ST_WOULD_PANIC with no record — and false when it goes on in the stripe to the left: p is then where (c0 == 0: never).
// kLocal: the walk stops at a cell with H == 0.  Every value that steers it comes out of a uniform load or a readlane, so the state
// is the same in all lanes; lane 0 writes.  The loop is bounded: a wrong direction word ends as ST_WOULD_PANIC, never as a hang.
template <bool kLocal>
__device__ __forceinline__ bool gap_walk(const GapArgs& a, int rd, int lane, int semi, int end_col, WalkPos& p, int c0, int C, int rows1) {
    const ReadState* rs = a.state + rd;
    DevRecord* rec = a.rec + rd;
    const int n = (int)(a.read_off[rd + 1] - a.read_off[rd]);
    const int pbeg = a.poff[rs->fwd_path], m = a.poff[rs->fwd_path + 1] - pbeg;
    const uint32_t* dirs = a.dirs + (long long)rd * a.dirs_stride;
    uint8_t* ops = a.ops + (long long)rd * a.ops_stride;
    uint32_t wd[4] = {0, 0, 0, 0};
    int i = p.i, j = p.j, state = p.state, nops = p.nops, steps = p.steps, have = -1;
    // Iterations of a valid walk.  A D is one (H: emit, i and j move).  A U is at most two: "H -> Y", then "Y: emit, i moves".  An L is
    // at most THREE: "H -> X", "X: emit, j moves", "arrive: back to H or on in X" — and with o == 0 every arrival goes back to H
    // (h + o >= x always holds), so a run of g L's takes 3 g.  Every emitted op moves i or j down, from at most (rows, n): at most
    // 2 per row + 3 per column, and one more for the stop.  3 (rows + n) + 3 covers it (counted over all the stripes of a walk).
    const int cap = 3 * (m + n) + 3;
    const int cs = 31 - __clz(C);                  // (C is a power of two)
    bool stopped = false;
    auto emit = [&](uint8_t op) { if (lane == 0 && nops < a.ops_stride) ops[nops] = op; ++nops; };
    while (i > 0 && j > 0 && j >= c0 && steps < cap) {
        ++steps;
        const uint32_t cell = dir_cell(dirs, C, cs, rows1, lane, i, j - c0, have, wd);
        if (state == S_XARRIVE) {                   // an L was walked into (i, j): does the run open here?
            state = (cell & 8u) ? S_H : S_X;
        } else if (state == S_H) {
            const uint32_t src = cell & 3u;
            if (kLocal && src == 0u) { stopped = true; break; }          // H == 0: checked first
            if (src == 1u) { emit(OP_D); i -= 1; j -= 1; }
            else state = src == 2u ? S_Y : S_X;
        } else if (state == S_Y) {
            emit(OP_U);
            i -= 1;
            state = (cell & 4u) ? S_H : S_Y;
        } else {
            emit(OP_L);
            j -= 1;
            state = S_XARRIVE;
        }
    }
    if (!stopped && i > 0 && j > 0) {
        if (steps >= cap) { no_record(rec, lane, ST_WOULD_PANIC); return true; }
        p = WalkPos{i, j, state, nops, steps};      // the column left the stripe
        return false;
    }
    if (kLocal) {
        // a border cell is H = 0 (X and Y are NEG there): the walk may arrive in H, or by an L whose run opens on column 0
        const bool border = (i == 0 || j == 0) && (state == S_H || (state == S_XARRIVE && j == 0));
        if (!(stopped || border) || nops < 1 || nops > a.ops_stride) { no_record(rec, lane, ST_WOULD_PANIC); return true; }
    } else {
        // the borders: only one state is finite there, and no direction word is needed
        while (j > 0) { emit(OP_L); j -= 1; }
        while (!semi && i > 0) { emit(OP_U); i -= 1; }
        if (nops > a.ops_stride) { no_record(rec, lane, ST_WOULD_PANIC); return true; }
    }
    write_record(rec, lane, rs, end_col, kLocal && i > 0 ? a.prow[pbeg + i - 1] : 0, kLocal ? j : 0, nops);
    return true;
}

// One wave per read: the whole walk in one launch, over a buffer of S stripes of 64 C columns (the single-wave kernels: S = 1), from
// (end row, last column) — local: from (end row, ReadState::rec_col) — to the record
template <bool kLocal>
__device__ __forceinline__ void gap_trace_wave(const GapArgs& a, int semi, int C, int S, int rows1) {
    const int rd = blockIdx.x, lane = threadIdx.x;
    const ReadState* rs = a.state + rd;
    DevRecord* rec = a.rec + rd;
    if (rs->status & ST_NO_RECORD) { no_record(rec, lane, rs->status); return; }
    const int n = (int)(a.read_off[rd + 1] - a.read_off[rd]);
    const int k = rs->fwd_path;
    const int pbeg = a.poff[k];
    const int idx = row_index(a.prow + pbeg, a.poff[k + 1] - pbeg, rs->end_row);
    const int end_col = kLocal ? rs->rec_col : n;
    if (idx < 0 || idx + 1 >= rows1 || n + 1 > S * C * WAVE || (kLocal && (end_col < 1 || end_col > n))) { no_record(rec, lane, ST_WOULD_PANIC); return; }
    WalkPos p{idx + 1, end_col, S_H, 0, 0};
    gap_walk<kLocal>(a, rd, lane, semi, end_col, p, 0, C, rows1);
}

// ---- launchers: the two dispatches (inside a launcher with `C` / `kind`, `s` and the kernel's arguments behind the grid; every case
// returns the launched instantiation's name, an unknown C / kind returns null) -------------------------------------------------------
// TAIL: the template arguments behind C, in parentheses: (, true) / ()
#define RG_GAP_SWITCH_C(K, TAIL, grid, ...) RG_SWITCH_C((4, 8, 16, 32), K, TAIL, grid, dim3(WAVE), 0, s, __VA_ARGS__)
#define RG_GAP_SWITCH_KIND(K, grid, ...)                                                        \
    do {                                                                                        \
        switch (kind) {                                                                         \
            case GAP_GLOBAL: RG_LAUNCH(K, (0), grid, dim3(WAVE), 0, s, __VA_ARGS__);            \
            case GAP_SEMI: RG_LAUNCH(K, (1), grid, dim3(WAVE), 0, s, __VA_ARGS__);              \
            case GAP_LOCAL: RG_LAUNCH(K, (2), grid, dim3(WAVE), 0, s, __VA_ARGS__);             \
            default: return nullptr;                                                            \
        }                                                                                       \
    } while (0)
