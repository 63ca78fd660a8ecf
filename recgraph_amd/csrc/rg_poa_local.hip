// Local POA kernels for gfx950: -m 1 in both of the reference's flavours (local_poa::exec_simd,
// src/local_poa.rs:9-174, and local_poa::exec, :176-262) and -m 3 (gap_local_poa::exec, src/gap_local_poa.rs:6-183),
// with the traceback of their GAF walkers (gaf_output.rs:383-752).
//
// The local modes are unbanded: the reference fills full L x W matrices.  Mapping as in rg_poa.hip: one wavefront per
// read, lanes over 64 consecutive columns of a row, rows sequential, every row written to HBM once (a later row may
// name any earlier row as predecessor).  The left recurrence, including the clamp at zero, is a wave-level max-plus
// prefix scan:
//   -m 1:  v[c] = max(b'[c], v[c-1] + g[c]),  b' = max(b, 0) where the reference clamps (its AVX2 multi-predecessor
//          tail does not), b = best of diagonal / up;
//   -m 3:  x[c] = e + max(x[c-1], m[c-1] + o) = e*c + max_{k<c}(t'[k] + o - e*k)  (o <= 0),  t' = max(d, y, 0).
// The direction of each cell is then re-derived from (d, u, l) with the reference's literal tie and clamp rules.
#include "rg_poa_common.hpp"

namespace rg {

// kVar 0: -m 1 AVX2 semantics (f32 values are integers < 2^24: int32 is exact);  1: -m 1 scalar;  2: -m 3.
// Planes per read (cap_cells each): m | y (kVar 2);  path words: w0 = pred << 3 | dir | X << 31,  w1 = predY << 1 | Y.
template <int kVar, bool kLdsRead>
__global__ __launch_bounds__(64) void k_poa_local(PoaArgs a) {
    extern __shared__ int pl_lds[];
    PoaRead<kLdsRead> P;
    if (!P.init(a, pl_lds, kVar == 2 ? 2 : 1)) return;
    const int rd = P.rd, lane = P.lane, W = P.W;
    const int* sct = P.sct;
    DevRecord* rec = P.rec;
    int *am = P.am, *ay = P.ay;
    uint32_t *pw0 = P.pw0, *pw1 = P.pw1;
    const DevLnz& g = a.g;
    const int L = g.L;
    if ((long long)(L - 1) * W > a.cap_cells) {
        if (lane == 0) { rec->status = ST_OVERFLOW; rec->n_ops = 0; }
        return;
    }
    const int o = a.gap_open, e = a.gap_ext;
    const int max_multiple = W % 8 != 0 ? (W / 8) * 8 : W - 8;   // local_poa.rs:19-23

    // row 0: all zero, path 'O' (local_poa.rs:17-18, :190-192)
    for (int c = lane; c < W; c += WAVE) {
        am[c] = 0; pw0[c] = 0;
        if (kVar == 2) { ay[c] = 0; pw1[c] = 0; }
    }
    __syncthreads();

    // best cell: kVar 0 takes the LAST maximum in row-major order ('>=', cells i,c >= 1 only, start (0,0));
    // kVar 1/2 take the FIRST ('>', all cells, start (0,0)).  Per lane (value, row-major index): a lane visits its cells in
    // increasing index order, so '>=' / '>' keep its last / first maximum; the wave then takes the largest value and, among
    // the lanes that hold it, the largest / smallest index.  (Value and index were packed into one 64-bit key with the
    // index in the low 40 bits: values of 2^23 and more wrapped, and local scores are i32 up to 2^31 in the reference.)
    int best_v = 0;
    long long best_i = 0;

    // The row above travels in registers (chunk k, lane l = column 64 k + l: local rows are full width, so chunks line
    // up) when W <= 64 KC: a row whose only predecessor is the row above needs no load and no barrier.
    constexpr int KC = 8;
    int pvm[KC] = {}, pvy[kVar == 2 ? KC : 1] = {};
    const bool p_fit = W <= KC * WAVE;
    bool dirty = false;

    for (int i = 1; i + 1 < L; ++i) {
        const int pb = uload(g.pred_off + i), pe = uload(g.pred_off + i + 1);
        const bool nwp = pe > pb;
        const bool fast = p_fit && !nwp;         // (rows with a listed predecessor take the reference's other code path)
        if (!fast && dirty) { __syncthreads(); dirty = false; }
        const int li = uload_u8(g.lnz, i);
        const long long rowoff = (long long)i * W;
        int keep_m[KC] = {}, keep_y[kVar == 2 ? KC : 1] = {};
        int ci = 0;
        int carry_z = NEG, carry_G = 0;
        AffCarry ac{NEG, 0, 0};                // kVar 2: x and t' of the previous chunk's last column
        for (int cb = 0; cb < W; cb += WAVE, ++ci) {
            const int c = cb + lane;
            const bool act = c < W;
            const bool cell = act && c >= 1;
            // fast path: m[i-1][c], m[i-1][c-1] (and y[i-1][c]) from the registers of the row above
            int f_u = 0, f_d = 0, f_y = 0;
            if (fast) {
                int cur_m = pvm[0], prv_m = 0, cur_y = pvy[0];
#pragma unroll
                for (int k = 1; k < KC; ++k) {
                    cur_m = ci == k ? pvm[k] : cur_m;
                    prv_m = ci == k ? pvm[k - 1] : prv_m;
                    if (kVar == 2) cur_y = ci == k ? pvy[kVar == 2 ? k : 0] : cur_y;
                }
                f_u = cur_m; f_y = cur_y;
                f_d = dpp_shr1(cur_m, 0);
                const int edge = __builtin_amdgcn_readlane(prv_m, WAVE - 1);
                if (lane == 0) f_d = edge;
            }
            const int rc = cell ? P.at(c) : 4;
            int d = 0, u = 0, dp = 0, up = 0;
            int uy = 0, uyp = 0;                 // kVar 2: y candidate
            if (cell) {
                if (fast) {
                    d = f_d; u = f_u; dp = up = i - 1;
                    if (kVar == 2) { uy = f_y; uyp = i - 1; }
                } else if (!nwp) {
                    const long long po = (long long)(i - 1) * W + c;
                    d = am[po - 1]; u = am[po]; dp = up = i - 1;
                    if (kVar == 2) { uy = ay[po]; uyp = i - 1; }
                } else if (kVar == 0) {
                    // first predecessor initialises, strict '>' afterwards (local_poa.rs:61-75, :129-143)
                    int p = g.pred_rows[pb];
                    long long po = (long long)p * W + c;
                    d = am[po - 1]; u = am[po]; dp = up = p;
                    for (int q = pb + 1; q < pe; ++q) {
                        p = g.pred_rows[q];
                        po = (long long)p * W + c;
                        const int dv = am[po - 1], uv = am[po];
                        if (uv > u) { u = uv; up = p; }
                        if (dv > d) { d = dv; dp = p; }
                    }
                } else {
                    // get_best_d / get_best_u start from (0, row 0): `first` is initialised to false
                    // (local_poa.rs:263-298, gap_local_poa.rs:126-183)
                    for (int q = pb; q < pe; ++q) {
                        const int p = g.pred_rows[q];
                        const long long po = (long long)p * W + c;
                        const int dv = am[po - 1];
                        if (dv > d) { d = dv; dp = p; }
                        if (kVar == 1) {
                            const int uv = am[po];
                            if (uv > u) { u = uv; up = p; }
                        } else {
                            const int um = am[po] + o, yv = ay[po];
                            if (um > u) { u = um; up = p; }
                            if (yv > uy) { uy = yv; uyp = p; }
                        }
                    }
                }
            }
            int mval = 0;
            uint32_t w0 = 0, w1 = 0;
            if (kVar == 0) {
                // ---------------- AVX2 flavour ----------------
                const bool simd = c <= max_multiple;
                int b = 0, gk = 0;
                bool isd = false, clamp = true;
                if (cell) {
                    const int us = u + sct[(li) * 6 + (GAP)];
                    if (simd) {
                        const int ds = d + sct[(li) * 6 + (rc)];
                        isd = ds > us;                                  // ties -> up (:47, :80)
                        b = isd ? ds : us;
                        gk = sct[(P.at(((c - 1) / 8) * 8 + 1)) * 6 + (GAP)];  // gap key of the chunk head (:94)
                    } else {
                        const int ds = d + (nwp ? sct[(rc) * 6 + (li)] : sct[(li) * 6 + (rc)]);   // swapped key (:147)
                        isd = ds >= us;                                 // D > U > L (:119-127, :150-156)
                        b = isd ? ds : us;
                        gk = sct[(rc) * 6 + (GAP)];
                        clamp = !nwp;                                   // the multi-predecessor tail never clamps
                    }
                }
                const int bsrc = !act ? NEG : (!cell ? 0 : (clamp ? max(b, 0) : b));
                const int G = dpp_incl_sum(gk) + carry_G;
                const LinScan z = lin_scan(bsrc, G, act, NEG, lane, carry_z);
                if (cell) {
                    const int l = z.zprev + G;
                    int v; uint32_t w;
                    if (l > b) { v = l; w = ((uint32_t)i << 3) | PD_L; }
                    else { v = b; w = isd ? (((uint32_t)dp << 3) | PD_D) : (((uint32_t)up << 3) | PD_U); }
                    if (clamp && (simd ? v <= 0 : v < 0)) { v = 0; w = 0; }   // '<= 0' (:99) vs '< 0' (:115)
                    mval = v; w0 = w;
                    if (v >= best_v) { best_v = v; best_i = rowoff + c; }
                }
                carry_G = lin_carry(z, G, carry_z);
            } else if (kVar == 1) {
                // ---------------- scalar flavour ----------------
                int dv = 0, uv = 0, gk = 0;
                if (cell) {
                    dv = d + sct[(rc) * 6 + (li)];            // key (sequence[j], lnz[i]) (:205, :213)
                    uv = u + sct[(GAP) * 6 + (li)];           // key ('-', lnz[i])
                    gk = sct[(rc) * 6 + (GAP)];
                }
                const int bsrc = !act ? NEG : (!cell ? 0 : max(max(dv, uv), 0));
                const int G = dpp_incl_sum(gk) + carry_G;
                const LinScan z = lin_scan(bsrc, G, act, NEG, lane, carry_z);
                if (cell) {
                    const int l = z.zprev + G;
                    const Cell r = pick_dul(dv, uv, l, ((uint32_t)(dp & 0xffff) << 3) | (li != rc ? PD_d : PD_D), ((uint32_t)(up & 0xffff) << 3) | PD_U,
                                            ((uint32_t)(i & 0xffff) << 3) | PD_L);           // utils.rs:129-140
                    if (!(dv < 0 && l < 0 && uv < 0)) { mval = r.v; w0 = r.w; }                  // else 0, 'O'
                    if (mval > best_v) { best_v = mval; best_i = rowoff + c; }
                }
                carry_G = lin_carry(z, G, carry_z);
            } else {
                // ---------------- -m 3 ----------------
                int dv = 0, yval = 0, ypred = 0, tcur = 0;
                bool fromy = false;
                if (cell) {
                    dv = d + sct[(rc) * 6 + (li)];
                    if (!nwp) {
                        const int u_y = uy + e, u_m = u + o + e;          // (:53-66)
                        fromy = u_y > u_m;
                        yval = fromy ? u_y : u_m;
                        ypred = i - 1;
                    } else {
                        const bool from_m = u > uy;                        // get_best_u (:177-182): u already holds m + o
                        yval = (from_m ? u : uy) + e;
                        ypred = from_m ? up : uyp;
                        fromy = !from_m;
                    }
                    tcur = max(max(dv, yval), 0);
                }
                // x[c] - e*c = max_{k<c} src[k] - e*k,  src[0] = x[0] = 0,  src[k] = t'[k] + o
                const int zsrc = !act ? NEG : ((cell ? tcur + o : 0) - e * c);
                AffScan x;
                x.zi = dpp_incl_max(zsrc, NEG);
                int ze = dpp_shr1(x.zi, NEG);
                ze = lane == 0 ? ac.z : max(ze, ac.z);
                x.xval = cell ? ze + e * c : 0;
                x.xprev = dpp_shr1(x.xval, 0); x.tprev = dpp_shr1(tcur, 0);
                if (lane == 0) { x.xprev = ac.x; x.tprev = ac.t; }
                if (cell) {
                    const bool xflag = o != 0 && x.xprev > x.tprev + o;       // path_x = 'X' iff x[c-1] + e > m[c-1] + o + e
                    const int l = x.xval, uu = yval;
                    const Cell r = pick_dul(dv, uu, l, ((uint32_t)(dp & 0xffff) << 3) | (li != rc ? PD_d : PD_D), ((uint32_t)(ypred & 0xffff) << 3) | PD_U,
                                            ((uint32_t)(i & 0xffff) << 3) | PD_L);
                    if (!(dv < 0 && l < 0 && uu < 0)) { mval = r.v; w0 = r.w; }
                    if (xflag) w0 |= X_BIT;
                    w1 = fromy ? (((uint32_t)(ypred & 0xffff) << 1) | 1u) : 0u;
                    if (mval > best_v) { best_v = mval; best_i = rowoff + c; }
                }
                if (act) ay[rowoff + c] = cell ? yval : 0;
#pragma unroll
                for (int k = 0; k < KC; ++k) keep_y[kVar == 2 ? k : 0] = ci == k ? (cell ? yval : 0) : keep_y[kVar == 2 ? k : 0];
                if (act) pw1[rowoff + c] = w1;
                aff_carry(x, tcur, ac);
            }
            if (act) { am[rowoff + c] = mval; pw0[rowoff + c] = w0; }
#pragma unroll
            for (int k = 0; k < KC; ++k) keep_m[k] = ci == k ? mval : keep_m[k];
        }
#pragma unroll
        for (int k = 0; k < KC; ++k) { pvm[k] = keep_m[k]; if (kVar == 2) pvy[kVar == 2 ? k : 0] = keep_y[kVar == 2 ? k : 0]; }
        dirty = true;
    }
    __syncthreads();
    const int bestv = (int)wave_max_ll(best_v);
    const long long held = kVar == 0 ? best_i : -best_i;          // kVar 1/2: the smallest index is the largest -index
    const long long bsel = wave_max_ll(best_v == bestv ? held : (long long)INT64_MIN);
    if (lane != 0) return;
    const long long bidx = kVar == 0 ? bsel : -bsel;
    const int best_row = (int)(bidx / W), best_col = (int)(bidx % W);

    // ---- traceback (gaf_output.rs:404-453, :527-598, :662-717), one lane ----
    const FullWidth cells{{}, pw0, pw1, W, L};
    OpsOut out(a, rd);
    int row = best_row, col = best_col;
    const uint32_t status = walk_trace<kVar == 2>(cells, L, W, row, col, out);
    write_record(rec, status, bestv, best_row, best_col, row, col, (status & ST_WOULD_PANIC) ? 0 : out.n);
    atomicAdd(a.cells, (unsigned long long)(L - 2) * (unsigned long long)(W - 1));
}

template <int kVar>
static const char* launch_local_v(const PoaArgs& a, hipStream_t s) {
    RG_POA_LAUNCH(k_poa_local, (kVar, true), (kVar, false), a, s);
}
const char* launch_local(const PoaArgs& a, int variant, hipStream_t s) {
    if (variant == 0) return launch_local_v<0>(a, s);
    if (variant == 1) return launch_local_v<1>(a, s);
    return launch_local_v<2>(a, s);
}

}  // namespace rg
