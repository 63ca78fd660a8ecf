// Bit-vector edit-distance pathwise alignment on BOTH STRANDS for gfx950 (-m 64 global, -m 65 semiglobal): the rule of -m 26 / -m 27 at
// unit costs (RG_MODE_PATHWISE_EDIT_STRANDS in include/recgraph_hip.h states it, and why "every read on both strands, reverse only if
// strictly greater" is the `< 0` gate of those modes here).  The score pass and the decision are this file's; the direction pass and the
// walk are k_edit_dirs / k_edit_trace of edit/rg_path_edit.hip, run once per read on the strand that won.
//
//   k_edit_score_pair<W, kSemi>   one wave per (read, path) scores BOTH strands: the last-column value of the path (-m 65: its best over the
//                                 rows, and the first row that attains it) -> ReadState::sink_val / path_end_row of state[rd] (the read as
//                                 given) and of state2[rd] (its reverse complement)
//   k_gap_pick                    the kernel of gap/rg_path_gap.hip, unchanged, once on `state` and once on `state2`
//   k_edit_strands_duel           one lane per read: the reverse pick replaces the forward one where it has a record and a STRICTLY greater
//                                 score; the strand byte says which strand that is
//
// LAYOUT.  A strand takes HALF A WAVE: lane l < 32 owns chunk l of the read as given, lane l >= 32 chunk l - 32 of the reverse complement,
// whose position t is the complement of read[n - 1 - t] (3 - c for c < 4, N stays) and is built from the forward bases while Peq is loaded:
// no reverse-complemented buffer.  Within a half, edit/rg_path_edit.hip's layout: bit t = column t + 1 in lane-of-half t / (32 W), word
// (t / 32) % W, bit t % 32; W = 1, 2, 4, 8 or 16 is the smallest with n <= 1024 W for the longest read of the batch.  So both strands of a
// read of at most 1024 W bases cost ONE row step of W words.
//
// THE ROW STEP is edit/rg_edit_bits.hpp's on every lane's chunk; the two cross-lane pieces are edit_strands/rg_edit_pair_bits.hpp's: the
// carries of the wide addition are two independent 32-bit chains on the halves of the two ballots, and lane 32 shifts in the border (hin
// into Ph, 0 into Mh) as lane 0 does — dpp_shr1 stays wave-wide and a select overrides the first lane of either half.
//
// THE SCORE of column n is tracked in each half by the lane that owns bit n - 1, as in k_edit_score.
#include <type_traits>

#include "rg_edit_pair_bits.hpp"
#include "rg_edit_strands.hpp"

namespace rg {

namespace {

#include "../gap/rg_path_gap_common.hpp"           // GNEG

#include "../edit/rg_path_edit_lane.hpp"            // load_match_bits, EditLane<W>

constexpr int DUEL_THREADS = 256;

// Peq of the lane's chunk of ITS strand's sequence, Pv all ones, Mv 0 (row 0 is 0, 1, 2, ...): EditLane<W>::load with the position
// mapped through the strand.  Every index into `read` lies in [0, n)
template <int W>
__device__ __forceinline__ void load_pair(EditLane<W>& st, const uint8_t* read /* read[0 .. n) */, int n, int lane, const int* mbits) {
    const bool rev = lane >= EDIT_PAIR_HALF;
    const int hl = lane & (EDIT_PAIR_HALF - 1);
#pragma unroll
    for (int k = 0; k < W; ++k) {
        uint32_t e0 = 0, e1 = 0, e2 = 0, e3 = 0, e4 = 0;
        const int c0 = (hl * W + k) * 32;
#pragma unroll 8
        for (int t = 0; t < 32; ++t) {
            int m = 0;
            if (c0 + t < n) {
                const int c = rev ? read[n - 1 - (c0 + t)] & 7 : read[c0 + t] & 7;
                m = mbits[rev && c < 4 ? 3 - c : c];
            }
            e0 |= (uint32_t)(m & 1) << t;
            e1 |= (uint32_t)((m >> 1) & 1) << t;
            e2 |= (uint32_t)((m >> 2) & 1) << t;
            e3 |= (uint32_t)((m >> 3) & 1) << t;
            e4 |= (uint32_t)((m >> 4) & 1) << t;
        }
        st.peq[0][k] = e0; st.peq[1][k] = e1; st.peq[2][k] = e2; st.peq[3][k] = e3; st.peq[4][k] = e4;
        st.pv[k] = ~0u;
        st.mv[k] = 0;
    }
}

}  // namespace

template <int W, bool kSemi>
__global__ __launch_bounds__(64) void k_edit_score_pair(GapArgs a, ReadState* state2) {
    __shared__ int mbits[8];
    const int rd = blockIdx.y, k = blockIdx.x, lane = threadIdx.x;
    const int hl = lane & (EDIT_PAIR_HALF - 1);
    const long long ro = a.read_off[rd];
    const int n = __builtin_amdgcn_readfirstlane((int)(a.read_off[rd + 1] - ro));
    if (a.bad[rd] || n < 1 || n > 32 * W * EDIT_PAIR_HALF) return;     // (the pick kernel reports a bad read, the direction pass one that is too long)
    const int pbeg = a.poff[k], m = a.poff[k + 1] - pbeg;
    load_match_bits(a, lane, mbits);
    EditLane<W> st;
    load_pair<W>(st, a.reads + ro, n, lane, mbits);
    // the bit of column n: in one word of one lane of either half, 0 everywhere else
    uint32_t nm[W];
#pragma unroll
    for (int w = 0; w < W; ++w) nm[w] = (hl == (n - 1) / (32 * W) && w == ((n - 1) / 32) % W) ? 1u << ((n - 1) % 32) : 0u;
    constexpr uint32_t hin = kSemi ? 0u : 1u;        // the border: column 0 is i (global) or 0 (semiglobal)
    int cur = n;                                     // the distance of column n, row 0
    int best = GNEG, bt = 0;
    // the bases of 64 path rows per gather, as k_edit_score does
    for (int t0 = 0; t0 < m; t0 += WAVE) {
        int myb = 4;
        if (t0 + lane < m) myb = a.lnz[a.prow[pbeg + t0 + lane]];
        const int cnt = min(WAVE, m - t0);
        for (int u = 0; u < cnt; ++u) {
            const int b = __builtin_amdgcn_readlane(myb, u);
            uint32_t eq[W], sum[W], ph[W], mh[W], d0[W];
            st.match(b, eq);
            const uint32_t g = edit_sum<W>(eq, st.pv, sum);
            const bool p = edit_chunk_all_ones<W>(sum);
            const uint64_t cm = edit_pair_carry_mask(__ballot(g != 0), __ballot(p));
            edit_deltas<W>(eq, st.pv, st.mv, sum, (uint32_t)(cm >> lane) & 1u, ph, mh, d0);
            uint32_t up = 0, dn = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) { up |= ph[w] & nm[w]; dn |= mh[w] & nm[w]; }
            cur += (up != 0 ? 1 : 0) - (dn != 0 ? 1 : 0);
            if (kSemi && -cur > best) { best = -cur; bt = t0 + u; }      // strictly better: the first row that attains the maximum
            const uint32_t pin = edit_pair_shift_in((uint32_t)dpp_shr1((int)(ph[W - 1] >> 31), (int)hin), lane, hin);
            const uint32_t nin = edit_pair_shift_in((uint32_t)dpp_shr1((int)(mh[W - 1] >> 31), 0), lane, 0u);
            edit_finish<W>(eq, st.pv, st.mv, ph, mh, pin, nin);
        }
    }
    if (hl == (n - 1) / (32 * W)) {
        ReadState* rs = (lane >= EDIT_PAIR_HALF ? state2 : a.state) + rd;
        rs->sink_val[k] = kSemi ? best : -cur;
        if (kSemi) rs->path_end_row[k] = m > 0 ? a.prow[pbeg + bt] : 0;
    }
    if (lane == 0) {
        const unsigned long long c = 2ull * (unsigned long long)m * (unsigned long long)n;      // both strands
        atomicAdd(a.cells, c);
        atomicAdd(a.cells + 1, c);
    }
}

// The strand rule on the two picks of a read: forward stays unless the reverse pick has a record and a STRICTLY greater score (ties and
// reverse palindromes: '+').  A read with a bad base — or without a forward record — keeps its forward state.  Where reverse wins, the
// fields gap_pick_wave writes (the ones k_gap_seed_pick lists) move from state2[rd] into state[rd]: all that the direction pass and the
// walk read of a pick.  The sink values of the forward strand stay where they are: nothing reads them again.
__global__ __launch_bounds__(DUEL_THREADS) void k_edit_strands_duel(ReadState* state, const ReadState* state2, uint8_t* strand, int nreads) {
    const int i = blockIdx.x * DUEL_THREADS + threadIdx.x;
    if (i >= nreads) return;
    ReadState* f = state + i;
    const ReadState* r = state2 + i;
    const bool rev = !(f->status & ST_NO_RECORD) && !(r->status & ST_NO_RECORD) && r->trace_score > f->trace_score;
    if (rev) {
        f->status = r->status;
        f->s0 = r->s0; f->bound = r->bound; f->trace_score = r->trace_score;
        f->seed_path = r->seed_path; f->fwd_path = r->fwd_path; f->rev_path = r->rev_path;
        f->end_row = r->end_row; f->end_row_best = r->end_row_best;
    }
    strand[i] = rev ? 1 : 0;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
const char* launch_edit_score_pair(const GapArgs& a, ReadState* state2, int nreads, int W, bool semi, hipStream_t s) {
    if (!a.state || !state2 || nreads < 1) return nullptr;
    const dim3 grid(a.P, nreads), block(WAVE);
#define RG_EDIT_PAIR_CASE_(w)                                                               \
    case w:                                                                                 \
        if (semi) RG_LAUNCH(k_edit_score_pair, (w, true), grid, block, 0, s, a, state2);    \
        else RG_LAUNCH(k_edit_score_pair, (w, false), grid, block, 0, s, a, state2);
    switch (W) {
        RG_EDIT_PAIR_CASE_(1)
        RG_EDIT_PAIR_CASE_(2)
        RG_EDIT_PAIR_CASE_(4)
        RG_EDIT_PAIR_CASE_(8)
        RG_EDIT_PAIR_CASE_(16)
        default: return nullptr;
    }
#undef RG_EDIT_PAIR_CASE_
}
const char* launch_edit_strands_duel(ReadState* state, const ReadState* state2, uint8_t* strand, int nreads, hipStream_t s) {
    if (!state || !state2 || !strand || nreads < 1) return nullptr;
    RG_LAUNCH0(k_edit_strands_duel, dim3((unsigned)((nreads + DUEL_THREADS - 1) / DUEL_THREADS)), dim3(DUEL_THREADS), 0, s, state, state2, strand, nreads);
}

}  // namespace rg
