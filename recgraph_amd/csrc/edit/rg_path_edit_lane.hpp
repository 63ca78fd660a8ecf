// What the kernel files of the bit-vector edit-distance modes share (edit/rg_path_edit.hip: -m 44 / -m 45; edit_xlong/rg_path_edit_xlong.hip:
// -m 94 / -m 95): the match table in LDS, one lane's chunk of the row state with the pieces of the row step (edit/rg_edit_bits.hpp)
// around their cross-lane exchanges, and the store of a row's D0 / Ph.  Everything here is inlined into its callers; included inside
// namespace rg, in each file's anonymous namespace, after edit/rg_edit_bits.hpp and gap/rg_path_gap.hpp (GapArgs).
#pragma once

// code of a read base -> bit b: the table scores path base b against it with 0 (codes 5 .. 7: nothing matches), in LDS
__device__ __forceinline__ void load_match_bits(const GapArgs& a, int lane, int* mbits) {
    if (lane < 8) {
        int m = 0;
#pragma unroll
        for (int b = 0; b < 5; ++b) m |= (lane < 5 && a.sc.t[b * 6 + (lane < 5 ? lane : 0)] == 0) ? 1 << b : 0;
        mbits[lane] = m;
    }
    __syncthreads();
}

// the lane's chunk of the row state, and the pieces of the row step around their cross-lane exchanges
template <int W>
struct EditLane {
    uint32_t peq[5][W], pv[W], mv[W];

    __device__ __forceinline__ void load(const uint8_t* read /* read[0 .. n) */, int n, int lane, const int* mbits) {
#pragma unroll
        for (int k = 0; k < W; ++k) {
            uint32_t e0 = 0, e1 = 0, e2 = 0, e3 = 0, e4 = 0;
            const int c0 = (lane * W + k) * 32;
#pragma unroll 8
            for (int t = 0; t < 32; ++t) {
                const int m = c0 + t < n ? mbits[read[c0 + t] & 7] : 0;
                e0 |= (uint32_t)(m & 1) << t;
                e1 |= (uint32_t)((m >> 1) & 1) << t;
                e2 |= (uint32_t)((m >> 2) & 1) << t;
                e3 |= (uint32_t)((m >> 3) & 1) << t;
                e4 |= (uint32_t)((m >> 4) & 1) << t;
            }
            peq[0][k] = e0; peq[1][k] = e1; peq[2][k] = e2; peq[3][k] = e3; peq[4][k] = e4;
            pv[k] = ~0u;
            mv[k] = 0;
        }
    }
    // Eq of path base b (wave-uniform): Peq[b], as five scalar masks of which one is all ones — an index would move Peq out of the
    // registers, and a chain of selects on the uniform b is compiled into a tree of scalar branches per word (two dozen scalar
    // instructions each).  The empty asm hides where a mask comes from, so that the AND stays an AND
    __device__ __forceinline__ void match(int b, uint32_t (&eq)[W]) const {
        uint32_t sel[5];
#pragma unroll
        for (int x = 0; x < 5; ++x) {
            int s = ((b ^ x) - 1) >> 31;            // b == x ? -1 : 0 (0 <= b <= 4), in scalar integer arithmetic
            asm("" : "+s"(s));
            sel[x] = (uint32_t)s;
        }
#pragma unroll
        for (int k = 0; k < W; ++k) eq[k] = (peq[0][k] & sel[0]) | (peq[1][k] & sel[1]) | (peq[2][k] & sel[2]) | (peq[3][k] & sel[3]) | (peq[4][k] & sel[4]);
    }
    // hin is -1, 0 or +1, wave-uniform: what column 0 of the vector did from the row above (THE STRIPED ROW STEP in edit/rg_edit_bits.hpp).
    // The unstriped kernels pass their border, +1 (global) or 0 (semiglobal), as a constant, and the lane-0 patch and the Mh term fold away.
    // The first two pieces: the chunk's sum, the carries of all lanes, Ph / Mh (unshifted) and D0.  Bit 0 of Eq, which is lane 0's, is
    // set for the Xh term where hin < 0; eq itself is left as it is
    __device__ __forceinline__ void deltas(uint32_t (&eq)[W], int hin, int lane, uint32_t (&ph)[W], uint32_t (&mh)[W], uint32_t (&d0)[W]) const {
        const uint32_t e0 = eq[0];
        eq[0] = lane == 0 ? edit_hin_eq0(e0, hin) : e0;
        uint32_t sum[W];
        const uint32_t g = edit_sum<W>(eq, pv, sum);
        const bool p = edit_chunk_all_ones<W>(sum);
        const uint64_t cm = edit_carry_mask(__ballot(g != 0), __ballot(p));
        edit_deltas<W>(eq, pv, mv, sum, (uint32_t)(cm >> lane) & 1u, ph, mh, d0);
        eq[0] = e0;
    }
    // the third piece (ph and mh come back shifted): lane 0 shifts (hin > 0) into Ph and (hin < 0) into Mh
    __device__ __forceinline__ void finish(const uint32_t (&eq)[W], int hin, uint32_t (&ph)[W], uint32_t (&mh)[W]) {
        const uint32_t pin = (uint32_t)dpp_shr1((int)(ph[W - 1] >> 31), (int)edit_hin_pin(hin));
        const uint32_t nin = (uint32_t)dpp_shr1((int)(mh[W - 1] >> 31), (int)edit_hin_nin(hin));
        edit_finish<W>(eq, pv, mv, ph, mh, pin, nin);
    }
};

// D0 and the unshifted Ph of a path row into row r = row index + 1 of the walk's buffer, coalesced as [r][2 W][lane] (edit/rg_path_edit.hpp)
template <int W>
__device__ __forceinline__ void store_row(uint32_t* out, int r, int lane, const uint32_t (&d0)[W], const uint32_t (&ph)[W]) {
    uint32_t* row = out + (long long)r * (2 * W * WAVE) + lane;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        row[w * WAVE] = d0[w];
        row[(W + w) * WAVE] = ph[w];
    }
}
