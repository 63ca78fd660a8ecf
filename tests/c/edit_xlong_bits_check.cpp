// CPU check of THE STRIPED ROW STEP of recgraph_amd/csrc/edit/rg_edit_bits.hpp (-m 94 / -m 95), with the very functions the kernels of
// edit_xlong/rg_path_edit_xlong.hpp call and in their order: a row of 2 or 3 stripes, each 64 chunks of W = 8 words with the ballots
// and the lane shifts done by hand, stripe s > 0 taking hin from the top bit of its left neighbour's unshifted Ph / Mh — against a plain
// row step on ONE wide integer over all stripes, whose addition carries across the seams.  Rows: random states in which whole chunks
// are all ones or all zero (every value of hin must occur at a seam), rows of random sequences from row 0 on, an all-match
// homopolymer, and a single mismatch at bit 16383 of stripe 0 and at bit 0 of stripe 1.  Built and run by
// tests/test_pathwise_edit_xlong_cpu.py.
#include <cstdint>
#include <random>
#include <vector>

#include "edit/rg_edit_bits.hpp"
#include "plan_check_common.hpp"

typedef std::vector<uint32_t> Wide;      // word 0 the lowest

constexpr int W = 8, L = 64, SW = W * L;      // words per stripe: 16384 bits

static Wide w_add(const Wide& a, const Wide& b) {
    Wide s(a.size());
    uint64_t c = 0;
    for (size_t k = 0; k < a.size(); ++k) {
        const uint64_t t = (uint64_t)a[k] + b[k] + c;
        s[k] = (uint32_t)t;
        c = t >> 32;
    }
    return s;
}
static Wide w_shl1(const Wide& a, uint32_t in) {
    Wide s(a.size());
    for (size_t k = 0; k < a.size(); ++k) {
        s[k] = (a[k] << 1) | in;
        in = a[k] >> 31;
    }
    return s;
}
template <class F>
static Wide w_map(const Wide& a, const Wide& b, const Wide& c, F f) {
    Wide s(a.size());
    for (size_t k = 0; k < a.size(); ++k) s[k] = f(a[k], b[k], c[k]);
    return s;
}

struct WideRow { Wide pv, mv, ph, mh, d0; };
// the unstriped row step as the header's comment writes it, on the whole vector; hin: the border's 0 or 1
static WideRow wide_step(const Wide& eq, const Wide& pv, const Wide& mv, uint32_t hin) {
    const Wide xv = w_map(eq, mv, mv, [](uint32_t e, uint32_t m, uint32_t) { return e | m; });
    const Wide sum = w_add(w_map(eq, pv, pv, [](uint32_t e, uint32_t p, uint32_t) { return e & p; }), pv);
    const Wide xh = w_map(sum, pv, eq, [](uint32_t s, uint32_t p, uint32_t e) { return (s ^ p) | e; });
    WideRow r;
    r.ph = w_map(mv, xh, pv, [](uint32_t m, uint32_t x, uint32_t p) { return m | ~(x | p); });
    r.mh = w_map(pv, xh, xh, [](uint32_t p, uint32_t x, uint32_t) { return p & x; });
    r.d0 = w_map(xh, mv, mv, [](uint32_t x, uint32_t m, uint32_t) { return x | m; });
    const Wide phs = w_shl1(r.ph, hin), mhs = w_shl1(r.mh, 0);
    r.pv = w_map(mhs, xv, phs, [](uint32_t m, uint32_t x, uint32_t p) { return m | ~(x | p); });
    r.mv = w_map(phs, xv, xv, [](uint32_t p, uint32_t x, uint32_t) { return p & x; });
    return r;
}

static int seen_hin[3];      // how often a stripe s > 0 took -1, 0, +1

// one stripe as EditLane<8>::deltas and finish take it with hin: words [w0, w0 + SW) of the vectors; returns what the next stripe takes
static int stripe_step(const Wide& eq, const Wide& pv, const Wide& mv, int w0, int hin, WideRow& r) {
    static uint32_t e[L][W], p[L][W], m[L][W], sum[L][W], ph[L][W], mh[L][W], d0[L][W];
    uint64_t G = 0, P = 0;
    for (int l = 0; l < L; ++l) {
        for (int k = 0; k < W; ++k) { e[l][k] = eq[w0 + l * W + k]; p[l][k] = pv[w0 + l * W + k]; m[l][k] = mv[w0 + l * W + k]; }
        if (l == 0) e[0][0] = rg::edit_hin_eq0(e[0][0], hin);      // for the Xh term only
        const uint32_t g = rg::edit_sum<W>(e[l], p[l], sum[l]);
        const bool ones = rg::edit_chunk_all_ones<W>(sum[l]);
        CHECK(!(g && ones));
        G |= (uint64_t)g << l;
        P |= (uint64_t)(ones ? 1 : 0) << l;
    }
    const uint64_t cm = rg::edit_carry_mask(G, P);      // (the carry out of lane 63 is dropped: it does not cross a stripe)
    for (int l = 0; l < L; ++l) rg::edit_deltas<W>(e[l], p[l], m[l], sum[l], (uint32_t)(cm >> l) & 1u, ph[l], mh[l], d0[l]);
    e[0][0] = eq[w0];                                     // Xv takes the real Eq
    const int hout = rg::edit_hout(ph[L - 1][W - 1], mh[L - 1][W - 1]);
    CHECK(!((ph[L - 1][W - 1] >> 31) & (mh[L - 1][W - 1] >> 31)));
    uint32_t pin[L], nin[L];
    for (int l = 0; l < L; ++l) {
        pin[l] = l == 0 ? rg::edit_hin_pin(hin) : ph[l - 1][W - 1] >> 31;
        nin[l] = l == 0 ? rg::edit_hin_nin(hin) : mh[l - 1][W - 1] >> 31;
        for (int k = 0; k < W; ++k) { r.ph[w0 + l * W + k] = ph[l][k]; r.mh[w0 + l * W + k] = mh[l][k]; r.d0[w0 + l * W + k] = d0[l][k]; }
    }
    for (int l = 0; l < L; ++l) {
        rg::edit_finish<W>(e[l], p[l], m[l], ph[l], mh[l], pin[l], nin[l]);
        for (int k = 0; k < W; ++k) { r.pv[w0 + l * W + k] = p[l][k]; r.mv[w0 + l * W + k] = m[l][k]; }
    }
    return hout;
}

// the whole row, stripe by stripe; the two masks of a 64-row block hold one row here (bit u = 5)
static WideRow striped_step(const Wide& eq, const Wide& pv, const Wide& mv, int S, uint32_t border) {
    const size_t N = eq.size();
    WideRow r;
    r.pv.resize(N); r.mv.resize(N); r.ph.resize(N); r.mh.resize(N); r.d0.resize(N);
    int hin = (int)border;
    for (int s = 0; s < S; ++s) {
        if (s > 0) ++seen_hin[hin + 1];
        const int hout = stripe_step(eq, pv, mv, s * SW, hin, r);
        const uint64_t up = hout > 0 ? 1ull << 5 : 0, down = hout < 0 ? 1ull << 5 : 0;
        hin = rg::edit_hin_of_masks(up, down, 5);
        CHECK(hin == hout && rg::edit_hin_of_masks(up, down, 4) == 0);
    }
    return r;
}

static bool same(const WideRow& a, const WideRow& b) { return a.pv == b.pv && a.mv == b.mv && a.ph == b.ph && a.mh == b.mh && a.d0 == b.d0; }

// rows of sequences from row 0 on: Eq of every row from a random read over `alphabet` letters, (Pv, Mv) = (all ones, 0) to start with
static void check_sequences(std::mt19937_64& rng, int S, int alphabet, int rows, int mismatch_bit /* -1: none; all other bits match */) {
    const int N = S * SW;
    std::vector<Wide> peq(alphabet, Wide(N, 0u));
    for (int t = 0; t < N * 32; ++t) peq[mismatch_bit >= 0 ? 0 : (int)(rng() % alphabet)][t / 32] |= 1u << (t % 32);
    if (mismatch_bit >= 0) peq[0][mismatch_bit / 32] &= ~(1u << (mismatch_bit % 32));
    for (uint32_t border = 0; border < 2; ++border) {
        Wide p1(N, ~0u), m1(N, 0u), p2 = p1, m2 = m1;
        for (int row = 0; row < rows; ++row) {
            const Wide& eq = peq[mismatch_bit >= 0 ? 0 : (int)(rng() % alphabet)];
            const WideRow a = wide_step(eq, p1, m1, border), b = striped_step(eq, p2, m2, S, border);
            CHECK(same(a, b));
            p1 = a.pv; m1 = a.mv; p2 = b.pv; m2 = b.mv;
        }
    }
}

static void check_random_states(std::mt19937_64& rng, int S) {
    const int N = S * SW;
    for (int it = 0; it < 120; ++it) {
        Wide eq(N), pv(N), mv(N);
        // a chunk is random, all ones or all zero; Pv and Mv never share a bit (a column is not both one more and one less)
        auto fill = [&](Wide& v, int ones_in, int zero_in) {
            for (int l = 0; l < S * L; ++l) {
                const int kind = (int)(rng() % 8);
                for (int k = 0; k < W; ++k) v[l * W + k] = kind < ones_in ? ~0u : kind < ones_in + zero_in ? 0u : (uint32_t)rng();
            }
        };
        fill(eq, it % 4, 1);
        fill(pv, it % 5, 1);
        fill(mv, 0, 2);
        for (int k = 0; k < N; ++k) mv[k] &= ~pv[k];
        if (it == 0) { std::fill(eq.begin(), eq.end(), ~0u); std::fill(pv.begin(), pv.end(), ~0u); std::fill(mv.begin(), mv.end(), 0u); }      // the carry ripples through every seam
        if (it == 1) { std::fill(eq.begin(), eq.end(), 0u); std::fill(pv.begin(), pv.end(), ~0u); std::fill(mv.begin(), mv.end(), 0u); }
        if (it == 2) { std::fill(eq.begin(), eq.end(), 0u); std::fill(pv.begin(), pv.end(), 0u); std::fill(mv.begin(), mv.end(), ~0u); }      // every column went down: Ph all ones
        for (uint32_t border = 0; border < 2; ++border) {
            Wide p1 = pv, m1 = mv, p2 = pv, m2 = mv;
            for (int row = 0; row < 3; ++row) {
                const WideRow a = wide_step(eq, p1, m1, border), b = striped_step(eq, p2, m2, S, border);
                CHECK(same(a, b));
                p1 = a.pv; m1 = a.mv; p2 = b.pv; m2 = b.mv;
                for (int k = 0; k < N; ++k) eq[k] = (eq[k] << 7) | (eq[k] >> 25);
            }
        }
    }
}

int main() {
    CHECK(rg::edit_hin_eq0(6u, -1) == 7u && rg::edit_hin_eq0(6u, 0) == 6u && rg::edit_hin_eq0(6u, 1) == 6u);
    CHECK(rg::edit_hin_pin(1) == 1 && rg::edit_hin_pin(0) == 0 && rg::edit_hin_pin(-1) == 0);
    CHECK(rg::edit_hin_nin(1) == 0 && rg::edit_hin_nin(0) == 0 && rg::edit_hin_nin(-1) == 1);
    CHECK(rg::edit_hout(1u << 31, 0) == 1 && rg::edit_hout(0, 1u << 31) == -1 && rg::edit_hout(~0u >> 1, ~0u >> 1) == 0);
    std::mt19937_64 rng(94);
    for (int S : {2, 3}) {
        int before[3] = {seen_hin[0], seen_hin[1], seen_hin[2]};
        check_random_states(rng, S);
        // all three values of hin, forced by the random top bits of the stripes
        for (int v = 0; v < 3; ++v) CHECK(seen_hin[v] - before[v] >= 20);
        check_sequences(rng, S, 4, 24, -1);
        check_sequences(rng, S, 2, 24, -1);
        // the homopolymer: every bit matches, the diagonal crosses every seam going down (hin = -1 in the global kind)
        before[0] = seen_hin[0];
        check_sequences(rng, S, 1, 40, -1);
        CHECK(seen_hin[0] - before[0] >= 40 * (S - 1));
        // one mismatch on either side of the first seam
        check_sequences(rng, S, 1, 40, 16383);
        check_sequences(rng, S, 1, 40, 16384);
    }
    return finish("edit xlong bits ok");
}
