// Band-relative POA kernels for gfx950: -m 2 (gap_global_abpoa::exec, src/gap_global_abpoa.rs:11-250)
// and the scalar -m 0 (global_abpoa::exec, src/global_abpoa.rs:260-427), with their band check
// (band_ampl_enough) and traceback walkers (gaf_output.rs:96-381).
//
// Same mapping as rg_poa.hip: one wavefront per read, lanes over the band columns of a row, rows
// sequential.  Storage is band-relative like the reference (cell j of row i <-> absolute column
// left_i + j); predecessor columns are translated with left_i - left_p and a predecessor only
// contributes where its band covers the column.
//
// The two "left" recurrences are evaluated as wave-level prefix scans:
//   m0 scalar:  m[j] = max(du[j], m[j-1] + g(read[c]))            (du = max(d, u), L on strict '>')
//   m2:         x[j] = e + max(x[j-1], m[j-1] + o),  m[j] = max(t[j], x[j]),  t = max(d, y)
//               => x[j] - e*j = max(boundary, max_{k<j}(t[k] + o - e*k))      (needs o <= 0)
#include "rg_band.hpp"
#include "rg_poa_common.hpp"

namespace rg {

// band_plain (utils.rs:17-72, simd_version = false): rg_band.hpp

// kGap = false: scalar -m 0;  kGap = true: -m 2.
// Arena planes per read (cap_cells each): m | y (m2) ; path words: w0 = pred<<3 | dir | X<<31, w1 = predY<<1 | Y.
template <bool kGap, bool kLdsRead>
// (8 waves per SIMD — 64 VGPRs — were tried like in rg_poa.hip: 6 registers spill and config 3 loses 2-8 %: not bound by
// occupancy either.  profiles/r04_notes.md)
__global__ __launch_bounds__(64) void k_poa_banded(PoaArgs a) {
    extern __shared__ int pb_lds[];
    PoaRead<kLdsRead> P;
    if (!P.init(a, pb_lds, kGap ? 2 : 1)) return;
    const int rd = P.rd, lane = P.lane, W = P.W;
    const int* sct = P.sct;
    DevRecord* rec = P.rec;
    int *am = P.am, *ay = P.ay;
    uint32_t *pw0 = P.pw0, *pw1 = P.pw1;
    const DevLnz& g = a.g;
    const int L = g.L;
    int4* rinfo = a.rinfo + (long long)P.slot * L;
    const unsigned long long bta = (unsigned long long)a.bta[rd];
    const int o = a.gap_open, e = a.gap_ext;
    long long off = 0;
    unsigned long long ncells = 0;
    uint32_t status = 0;
    bool overflow = false;

    // The previous row travels in registers (chunk k, lane l holds band cell 64 k + l = column p_left + 64 k + l) when it
    // fits KC chunks: a row whose only predecessor is the row above then needs no load, no barrier, and its stores are
    // fire and forget.  Rows with other predecessors take the memory path; a barrier orders the earlier stores first.
    constexpr int KC = 8;
    int pvm[KC] = {}, pvy[kGap ? KC : 1] = {};
    int p_left = 0, p_right = 0, p_best = 0;
    bool p_valid = false, dirty = false;
    // (the empty asm statements keep the selects apart: left alone the compiler fuses a chain of them into a dynamically
    // indexed vector which it keeps in SCRATCH — 48 bytes per lane, stores every row and dependent loads every chunk of the
    // fast path; found in the ISA in round 4, see rg_poa.hip)
    auto chunk_of = [&](const int (&arr)[KC], int k) -> int {
        int r = arr[0];
#pragma unroll
        for (int kk = 1; kk < KC; ++kk) { r = k == kk ? arr[kk] : r; asm volatile("" : "+v"(r)); }
        return r;
    };

    // per-row metadata: one 16-byte scalar load, a row ahead (PoaArgs::rowmeta_b; as six loads at the top of the row — one of
    // them dependent — every row waited for the scalar cache several times)
    int n_pb = 0;
    int4 n_meta = uload4(a.rowmeta_b);
    for (int i = 0; i + 1 < L; ++i) {
        const int pb = n_pb, pe = n_meta.x, m_rv = n_meta.y, m_minp = n_meta.z, m_p0 = (n_meta.w & 0xffffff) - 1, m_li = n_meta.w >> 24;
        n_pb = pe;
        if (i + 2 < L) n_meta = uload4(a.rowmeta_b + i + 1);
        const bool nwp = pe > pb;
        const bool only_prev = i > 0 && (!nwp || (pe - pb == 1 && m_p0 == i - 1));
        unsigned long long ms = 0, me = 0;
        if (i > 0) {
            if (only_prev) { unsigned long long pl = (unsigned long long)p_best; ms = pl + 1; me = pl + 1; }
            else {
                if (dirty) { __syncthreads(); dirty = false; }
                unsigned long long pl = 0, pr = 0;
                for (int ee = pb; ee < pe; ++ee) {
                    unsigned long long cb = (unsigned long long)rinfo[g.pred_rows[ee]].w;
                    if (ee == pb) { pl = cb; pr = cb; }
                    if (cb < pl) pl = cb;
                    if (cb > pr) pr = cb;
                }
                ms = pl + 1; me = pr + 1;
            }
        }
        int left, right;
        band_plain(ms, me, m_rv, (unsigned long long)W, bta, left, right);
        if (right <= left) { status |= ST_WOULD_PANIC; break; }   // empty row: m[i][best_val_pos] out of range
        const int width = right - left;
        if (off + width > a.cap_cells) { overflow = true; break; }
        const int li = m_li;
        const int minp = m_minp;
        const bool fast = only_prev && p_valid && width <= KC * WAVE;
        if (i > 0 && !fast && dirty) { __syncthreads(); dirty = false; }
        int keep_m[KC] = {}, keep_y[kGap ? KC : 1] = {};
        int ci = 0;
        // carries of the scans across 64-column chunks
        int carry_z = NEG;        // m0 scalar: running prefix max (exclusive) of the scan variable
        int carry_G = 0;          // m0 scalar: prefix sum of gap costs
        AffCarry ac{NEG, NEG, NEG};   // m2
        long long best_key = ((long long)INT32_MIN) * 4294967296ll;
        for (int cb = 0; cb < width; cb += WAVE, ++ci) {
            const int j = cb + lane;
            const bool act = j < width;
            const int c = left + j;
            const int rc = (act && c >= 1) ? P.at(c) : 4;
            // fast path: m[i-1] at columns c-1 and c (and y[i-1] at c) from the registers of the row above
            int f_md = 0, f_mu = 0, f_yu = 0;
            if (fast) {
                const int k0 = (left + cb - 1 - p_left) >> 6;          // columns c-1 .. c of this chunk span chunks k0, k0+1
                const int ka = k0 < 0 ? 0 : (k0 < KC ? k0 : KC - 1), kb = k0 + 1 < 0 ? 0 : (k0 + 1 < KC ? k0 + 1 : KC - 1);
                const int mlo = chunk_of(pvm, ka), mhi = chunk_of(pvm, kb);
                // ONE cross-lane fetch per plane (round 6; two ds_bpermute per value and three values per chunk before).  The
                // lanes of a chunk read consecutive band cells: lane l reads cell base + l — a ROTATION of the lanes by
                // rot = base mod 64 over the two register chunks k0 (cells whose lane is >= rot) and k0 + 1 (the others).  So
                // the SOURCE lane selects which of its two chunk values is wanted (a lane is read exactly once), one
                // ds_bpermute rotates, and column c (the cell behind column c - 1) is the next lane's fetch: a one-lane wave
                // shift, with lane 63's value — cell base + 64: lane rot of chunk k0 + 1 — through a v_readlane.
                const int base = left + cb - 1 - p_left;               // band cell of column c - 1 for lane 0 (wave-uniform)
                const int rot = base & (WAVE - 1);
                const int rsel = ((rot + lane) & (WAVE - 1)) * 4;      // byte address of the lane ds_bpermute reads
                f_md = __builtin_amdgcn_ds_bpermute(rsel, lane >= rot ? mlo : mhi);
                {
                    const int last = __builtin_amdgcn_readlane(mhi, rot);
                    const int sh = dpp_mov<0x130, 0xf>(0, f_md);       // wave_shl:1 — lane l takes lane l + 1's value
                    f_mu = lane == WAVE - 1 ? last : sh;
                }
                if (kGap) {
                    int ylo = pvy[0], yhi = pvy[0];
#pragma unroll
                    for (int kk = 1; kk < (kGap ? KC : 1); ++kk) {
                        ylo = ka == kk ? pvy[kGap ? kk : 0] : ylo; yhi = kb == kk ? pvy[kGap ? kk : 0] : yhi;
                        asm volatile("" : "+v"(ylo), "+v"(yhi));
                    }
                    {
                        // column c of y: band cell base + 1 + l — the same rotation one cell further
                        const int rot1 = (base + 1) & (WAVE - 1);
                        const int rsel1 = ((rot1 + lane) & (WAVE - 1)) * 4;
                        const int k1 = (base + 1) >> 6;               // chunk of lane 0's cell; k1 == k0 except when rot == 63
                        // (rot == 63: base + 1 is a multiple of 64, every lane's cell lies in chunk k0 + 1 and every lane is >= rot1 = 0)
                        const int ylo1 = k1 == k0 ? ylo : yhi;
                        f_yu = __builtin_amdgcn_ds_bpermute(rsel1, lane >= rot1 ? ylo1 : yhi);
                    }
                }
            }
            const int first_prev = __builtin_amdgcn_readlane(pvm[0], 0);   // first stored cell of the row above
            // ---- candidates from the predecessor rows ----
            int d = 0, u = 0, dp = minp, up = minp;
            bool have_d = false, have_u = false;
            int uy = 0, uyp = minp;      // m2: best y of covering predecessors
            bool fixed = false;          // cell fully determined without the left chain
            int mval = 0;
            uint32_t w0 = 0, w1 = 0;
            int tval = NEG;             // non-left candidate of the cell (max(d,u) / max(d,y))
            uint32_t tw0 = 0;            // its path word
            int yval = 0;
            if (act) {
                if (i == 0 && j == 0) { fixed = true; mval = 0; w0 = PD_O; }
                else if (i == 0) {
                    if (kGap) { fixed = true; mval = o + e * c; yval = mval; w0 = (0u << 3) | PD_L; }
                    // scalar m0 row 0 is a pure left chain: handled by the scan with tval = NEG
                } else if (j == 0 && left == 0) {
                    fixed = true;
                    if (kGap) { mval = o + e * (minp + 1); w0 = ((uint32_t)minp << 3) | PD_U; }
                    else {
                        const int first = (fast && minp == i - 1) ? first_prev : am[rinfo[minp].x];
                        mval = first + sct[(GAP) * 6 + (li)];       // m[best_p][0] band-relative (:316)
                        w0 = ((uint32_t)minp << 3) | PD_U;
                    }
                } else if (fast) {
                    const int p = i - 1;
                    if (c > p_left && c <= p_right) { d = f_md; dp = p; have_d = true; }     // diagonal: left_p < c <= right_p
                    if (c >= p_left && c < p_right) {                                         // up: left_p <= c < right_p
                        if (kGap) { u = f_mu + o; up = p; uy = f_yu; uyp = p; }
                        else { u = f_mu; up = p; }
                        have_u = true;
                    }
                } else {
                    const int np = nwp ? pe - pb : 1;
                    for (int q = 0; q < np; ++q) {
                        const int p = nwp ? g.pred_rows[pb + q] : i - 1;
                        const int4 rp = rinfo[p];
                        if (c > rp.y && c <= rp.z) {                 // diagonal: left_p < c <= right_p
                            const int v = am[rp.x + (c - rp.y) - 1];
                            if (!have_d || v > d) { d = v; dp = p; }
                            have_d = true;
                        }
                        if (c >= rp.y && c < rp.z) {                 // up: left_p <= c < right_p
                            if (kGap) {
                                const int vm = am[rp.x + (c - rp.y)] + o, vy = ay[rp.x + (c - rp.y)];
                                if (!have_u) { u = vm; up = p; uy = vy; uyp = p; }
                                if (vm > u) { u = vm; up = p; }
                                if (vy > uy) { uy = vy; uyp = p; }
                            } else {
                                const int v = am[rp.x + (c - rp.y)];
                                if (!have_u || v > u) { u = v; up = p; }
                            }
                            have_u = true;
                        }
                    }
                }
            }
            if (!kGap) {
                // ---------------- scalar m0 (global_abpoa.rs:318-390) ----------------
                int gc = 0;
                bool chain = false;           // cell takes part in the left chain
                int lfb = NEG;               // left fallback of a band-left cell (:337-339)
                if (act && !fixed) {
                    if (i == 0) { chain = true; gc = sct[(GAP) * 6 + (rc)]; tval = NEG; }   // key ('-', base) (:307)
                    else {
                        const int dv = have_d ? d + sct[(li) * 6 + (rc)] : sct[(li) * 6 + (GAP)] * (i + left);
                        const int uv = have_u ? u + sct[(li) * 6 + (GAP)] : sct[(li) * 6 + (GAP)] * (i + left + j);
                        const int dpp = have_d ? dp : minp, upp = have_u ? up : minp;
                        if (dv < uv) { tval = uv; tw0 = ((uint32_t)(upp & 0xffff) << 3) | PD_U; }
                        else { tval = dv; tw0 = ((uint32_t)(dpp & 0xffff) << 3) | (rc != li ? PD_d : PD_D); }
                        gc = sct[(rc) * 6 + (GAP)];
                        if (j > 0) chain = true;
                        else lfb = sct[(rc) * 6 + (GAP)] * (i + left + j);
                    }
                }
                // scan: z = value - G
                const int G = dpp_incl_sum(act ? gc : 0) + carry_G;
                int v0 = tval;                // value of a cell as a chain SOURCE
                uint32_t v0w = tw0;
                if (fixed) { v0 = mval; v0w = w0; }
                if (act && !fixed && !chain && i > 0) {   // band-left cell with left > 0: l is a constant
                    if (lfb > tval) { v0 = lfb; v0w = ((uint32_t)(minp & 0xffff) << 3) | PD_L; }
                }
                const LinScan z = lin_scan(v0, G, act, NEG, lane, carry_z);
                if (act) {
                    int v = v0;
                    uint32_t w = v0w;
                    if (chain && z.zprev > z.y) { v = z.zprev + G; w = ((uint32_t)(i & 0xffff) << 3) | PD_L; }
                    if (chain && i == 0) { v = z.zprev + G; w = (0u << 3) | PD_L; }
                    am[off + j] = v;
                    pw0[off + j] = w;
                    mval = v;
                    // (no effect, and not dead weight: without this statement k_poa_banded<false, false> allocates 58 VGPRs instead of 57)
                    if (!fixed && i > 0) ncells += 0;
                }
                carry_G = lin_carry(z, G, carry_z);
#pragma unroll
                for (int k = 0; k < KC; ++k) { keep_m[k] = ci == k ? mval : keep_m[k]; asm volatile("" : "+v"(keep_m[k])); }
            } else {
                // ---------------- m2 (gap_global_abpoa.rs:67-196) ----------------
                const bool fixed0 = act && i > 0 && j == 0 && left == 0;   // first column (:78-92)
                const bool general = act && i > 0 && !fixed0;
                int dv = NEG, up_pred = minp, tcur = NEG, xb = NEG;
                bool fromy = false;
                if (act && i == 0) { mval = j == 0 ? 0 : o + e * c; yval = mval; w0 = j == 0 ? (uint32_t)PD_O : ((0u << 3) | PD_L); }
                if (fixed0) { mval = o + e * (minp + 1); xb = mval; w0 = ((uint32_t)(minp & 0xffff) << 3) | PD_U; yval = 0; }
                if (general) {
                    if (have_u) {                                   // get_best_u (:296-346)
                        if (uy > u) { yval = uy + e; up_pred = uyp; fromy = true; }
                        else { yval = u + e; up_pred = up; }
                    } else { yval = 2 * o + e * (minp + 1) + e * c; up_pred = minp; }   // (:139)
                    if (have_d) dv = d + sct[(li) * 6 + (rc)];
                    tcur = max(dv, yval);
                    if (j == 0) xb = 2 * o + e * (minp + 1) + e * c;                    // (:117)
                }
                // x[j] - e*j = max over k < j of max(t[k] + o, xb[k]) - e*k   (x[j] = e + max(x[j-1], m[j-1] + o), o <= 0)
                int zsrc = NEG;
                if (fixed0 || general) zsrc = max(tcur > NEG ? tcur + o : NEG, xb) - e * j;
                AffScan x;
                x.zi = dpp_incl_max(zsrc, NEG);
                int ze = dpp_shr1(x.zi, NEG);
                ze = lane == 0 ? ac.z : max(ze, ac.z);
                x.xval = NEG;
                if (fixed0 || general) x.xval = j == 0 ? xb : ze + e * j;
                x.xprev = dpp_shr1(x.xval, NEG); x.tprev = dpp_shr1(tcur, NEG);
                if (lane == 0) { x.xprev = ac.x; x.tprev = ac.t; }
                // path_x = 'X' iff x[j-1] > m[j-1] + o, i.e. (o < 0) x[j-1] > t[j-1] + o   (:350-368)
                const bool xflag = general && j > 0 && o != 0 && x.xprev > (x.tprev > NEG ? x.tprev + o : NEG);
                if (general) {
                    const int l = x.xval, uu = yval;
                    const uint32_t lpred = (uint32_t)((j > 0 ? i : minp) & 0xffff);
                    int mv; uint32_t w;
                    if (have_d) {                                    // (:145-180)
                        if (dv < l) {
                            if (l < uu) {
                                if (up_pred == 0) status |= ST_WOULD_PANIC;     // set_path_cell(_, 'u') panics
                                mv = uu; w = ((uint32_t)(up_pred & 0xffff) << 3) | PD_U;
                            } else { mv = l; w = (lpred << 3) | PD_L; }
                        } else {
                            if (dv < uu) { mv = uu; w = ((uint32_t)(up_pred & 0xffff) << 3) | PD_U; }
                            else { mv = dv; w = ((uint32_t)(dp & 0xffff) << 3) | (rc == li ? PD_D : PD_d); }
                        }
                    } else {                                         // (:181-194)
                        if (l < uu) { mv = uu; w = ((uint32_t)(up_pred & 0xffff) << 3) | PD_U; }
                        else { mv = l; w = (lpred << 3) | PD_L; }
                    }
                    mval = mv;
                    w0 = w | (xflag ? X_BIT : 0u);
                    w1 = fromy ? (((uint32_t)(up_pred & 0xffff) << 1) | 1u) : 0u;
                }
                if (act) {
                    am[off + j] = mval;
                    ay[off + j] = yval;
                    pw0[off + j] = w0;
                    pw1[off + j] = w1;
                }
                aff_carry(x, tcur, ac);
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    keep_m[k] = ci == k ? mval : keep_m[k];
                    asm volatile("" : "+v"(keep_m[k]));
                    if (kGap) { keep_y[kGap ? k : 0] = ci == k ? yval : keep_y[kGap ? k : 0]; asm volatile("" : "+v"(keep_y[kGap ? k : 0])); }
                }
            }
            // best_scoring_pos: last column attaining the row maximum
            const int cmx = __builtin_amdgcn_readlane(dpp_incl_max(act ? mval : INT32_MIN, INT32_MIN), WAVE - 1);
            if (cmx >= (int)(best_key >> 32)) {
                const unsigned long long at = __ballot(act && mval == cmx);
                best_key = (long long)cmx * 4294967296ll + (long long)(unsigned)(cb + 63 - __clzll((long long)at));
            }
        }
        // general cells of this row (reference's unit of work)
        {
            int general = 0;
            if (i > 0) general = width - (left == 0 ? 1 : 0);
            ncells += (unsigned long long)general;
        }
        if (lane == 0) rinfo[i] = make_int4((int)off, left, right, (int)(best_key & 0xffffffffll) + left);
        p_best = (int)(best_key & 0xffffffffll) + left; p_left = left; p_right = right;
        p_valid = width <= KC * WAVE;
#pragma unroll
        for (int k = 0; k < KC; ++k) { pvm[k] = keep_m[k]; if (kGap) pvy[kGap ? k : 0] = keep_y[kGap ? k : 0]; }
        off += width;
        dirty = true;
    }
    __syncthreads();
    // combine status bits raised by any lane
    for (int dd = WAVE / 2; dd >= 1; dd >>= 1) status |= __shfl_xor(status, dd, WAVE);
    if (overflow) {
        if (lane == 0) { rec->status = ST_OVERFLOW; rec->n_ops = 0; }
        return;
    }
    if (status & ST_WOULD_PANIC) {
        if (lane == 0) { rec->status = status; rec->n_ops = 0; rec->score = 0; }
        return;
    }
    if (lane != 0) return;

    // ---- end node (global_abpoa.rs:397-405, gap_global_abpoa.rs:206-214) ----
    int last_row = L - 2;
    int4 rl = rinfo[last_row];
    int last_col = rl.z - rl.y - 1;
    int bestv = am[rl.x + last_col];
    for (int ee = g.pred_off[L - 1]; ee < g.pred_off[L]; ++ee) {
        const int p = g.pred_rows[ee];
        const int4 rp = rinfo[p];
        const int tl = rp.z - rp.y - 1;
        const int v = am[rp.x + tl];
        if (v > bestv) { bestv = v; last_row = p; last_col = tl; }
    }
    const BandRel cells{pw0, pw1, rinfo};
    OpsOut out(a, rd);
    // ---- band_ampl_enough (global_abpoa.rs:428-476, gap_global_abpoa.rs:371-455) ----
    {
        int i = last_row, j = last_col;
        bool ok = true;
        int guard = 0;
        while (true) {
            if (++guard > 4 * (L + W)) { status |= ST_WOULD_PANIC; break; }
            if (i < 0 || i >= L - 1 || j < 0 || j >= cells.width(i)) { status |= ST_WOULD_PANIC; break; }
            const uint32_t w = cells.w0(i, j);
            const uint32_t dir = w & 7u;
            if (dir == PD_O) break;
            const int4 ri = rinfo[i];
            if (i == 0 || (j == 0 && ri.y == 0)) break;
            if ((j == 0 && ri.y != 0) || (j == ri.z - ri.y - 1 && ri.z != W)) { ok = false; break; }
            const int pred = (int)((w >> 3) & 0xffffu);
            if (dir == PD_D || dir == PD_d) {
                int jp;
                if (!cells.pred_col(i, j, pred, jp) || jp == 0) { status |= ST_WOULD_PANIC; break; }
                j = jp - 1; i = pred;
            } else if (dir == PD_L) {
                if (kGap && (w >> 31)) { while (j > 0 && j < cells.width(i) && (cells.w0(i, j) >> 31)) j -= 1; }
                else j -= 1;
            } else if (dir == PD_U) {
                if (kGap && (cells.w1(i, j) & 1u)) {
                    if (!walk_u_run<false>(cells, i, j, out)) { status |= ST_WOULD_PANIC; break; }
                } else {
                    int jp;
                    if (!cells.pred_col(i, j, pred, jp)) { status |= ST_WOULD_PANIC; break; }
                    j = jp; i = pred;
                }
            } else { if (kGap) { ok = false; } else { status |= ST_WOULD_PANIC; } break; }
        }
        if (!ok) status |= ST_BAND_WARNING;
    }
    // ---- traceback (gaf_output.rs:124-213 / 280-344) ----
    int row = last_row, col = last_col;
    if (!(status & ST_WOULD_PANIC)) status |= walk_trace<kGap>(cells, L, W, row, col, out);
    // query_end = last_col + left(last_row); query_start = the band-relative column where the walk stopped
    write_record(rec, status, bestv, last_row, last_col + rinfo[last_row].y, row, col, (status & ST_WOULD_PANIC) ? 0 : out.n);
    atomicAdd(a.cells, ncells);
}

template <bool kGap>
static const char* launch_banded(const PoaArgs& a, hipStream_t s) {
    RG_POA_LAUNCH(k_poa_banded, (kGap, true), (kGap, false), a, s);
}
const char* launch_m2(const PoaArgs& a, hipStream_t s) { return launch_banded<true>(a, s); }
const char* launch_m0_scalar(const PoaArgs& a, hipStream_t s) { return launch_banded<false>(a, s); }

}  // namespace rg
