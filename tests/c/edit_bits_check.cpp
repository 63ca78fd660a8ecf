// CPU check of recgraph_amd/csrc/edit/rg_edit_bits.hpp, the bit arithmetic of the edit-distance kernels (-m 44 / -m 45), with the very
// functions the kernels call: the carry mask against a bit-serial ripple (every (G, P) pair with G & P == 0 at 10 lanes, random 64-bit
// pairs), and the row step in its three pieces over 64 chunks of W = 1, 2, 4, 8 words — the ballots and the lane shifts done by hand —
// against a plain row step on one wide integer, on random vectors in which whole chunks are all ones or all zero.  Built and run by
// tests/test_pathwise_edit_cpu.py.
#include <cstdint>
#include <random>
#include <vector>

#include "edit/rg_edit_bits.hpp"
#include "plan_check_common.hpp"

typedef std::vector<uint32_t> Wide;      // word 0 the lowest

static uint64_t ripple_mask(uint64_t G, uint64_t P, int lanes) {
    uint64_t m = 0, c = 0;
    for (int l = 0; l < lanes; ++l) {
        m |= c << l;
        c = ((G >> l) & 1) | (((P >> l) & 1) & c);
    }
    return m;
}

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
// the row step as the header's comment writes it, on the whole vector
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

// the same step as the kernels take it: 64 lanes of W words
template <int W>
static WideRow lane_step(const Wide& eq, const Wide& pv, const Wide& mv, uint32_t hin) {
    constexpr int L = 64;
    uint32_t e[L][W], p[L][W], m[L][W], sum[L][W], ph[L][W], mh[L][W], d0[L][W];
    uint64_t G = 0, P = 0;
    for (int l = 0; l < L; ++l) {
        for (int k = 0; k < W; ++k) { e[l][k] = eq[l * W + k]; p[l][k] = pv[l * W + k]; m[l][k] = mv[l * W + k]; }
        const uint32_t g = rg::edit_sum<W>(e[l], p[l], sum[l]);
        const bool ones = rg::edit_chunk_all_ones<W>(sum[l]);
        CHECK(!(g && ones));
        G |= (uint64_t)g << l;
        P |= (uint64_t)(ones ? 1 : 0) << l;
    }
    const uint64_t cm = rg::edit_carry_mask(G, P);
    for (int l = 0; l < L; ++l) rg::edit_deltas<W>(e[l], p[l], m[l], sum[l], (uint32_t)(cm >> l) & 1u, ph[l], mh[l], d0[l]);
    WideRow r;
    r.pv.resize(L * W); r.mv.resize(L * W); r.ph.resize(L * W); r.mh.resize(L * W); r.d0.resize(L * W);
    uint32_t pin[L], nin[L];
    for (int l = 0; l < L; ++l) {
        pin[l] = l == 0 ? hin : ph[l - 1][W - 1] >> 31;
        nin[l] = l == 0 ? 0 : mh[l - 1][W - 1] >> 31;
        for (int k = 0; k < W; ++k) { r.ph[l * W + k] = ph[l][k]; r.mh[l * W + k] = mh[l][k]; r.d0[l * W + k] = d0[l][k]; }
    }
    for (int l = 0; l < L; ++l) {
        rg::edit_finish<W>(e[l], p[l], m[l], ph[l], mh[l], pin[l], nin[l]);
        for (int k = 0; k < W; ++k) { r.pv[l * W + k] = p[l][k]; r.mv[l * W + k] = m[l][k]; }
    }
    return r;
}

template <int W>
static void check_rows(std::mt19937_64& rng) {
    constexpr int N = 64 * W;
    for (int it = 0; it < 300; ++it) {
        Wide eq(N), pv(N), mv(N);
        // a chunk is random, all ones or all zero; Pv and Mv never share a bit (a column is not both one more and one less)
        auto fill = [&](Wide& v, int ones_in, int zero_in) {
            for (int l = 0; l < 64; ++l) {
                const int kind = (int)(rng() % 8);
                for (int k = 0; k < W; ++k) v[l * W + k] = kind < ones_in ? ~0u : kind < ones_in + zero_in ? 0u : (uint32_t)rng();
            }
        };
        fill(eq, it % 4, 1);
        fill(pv, it % 5, 1);
        fill(mv, 0, 2);
        for (int k = 0; k < N; ++k) mv[k] &= ~pv[k];
        if (it == 0) { std::fill(eq.begin(), eq.end(), ~0u); std::fill(pv.begin(), pv.end(), ~0u); std::fill(mv.begin(), mv.end(), 0u); }      // the carry ripples through every lane
        if (it == 1) { std::fill(eq.begin(), eq.end(), 0u); std::fill(pv.begin(), pv.end(), ~0u); std::fill(mv.begin(), mv.end(), 0u); }
        if (it == 2) { std::fill(eq.begin(), eq.end(), ~0u); eq[0] = 1; std::fill(pv.begin(), pv.end(), ~0u); pv[0] = ~0u; std::fill(mv.begin(), mv.end(), 0u); }
        for (uint32_t hin = 0; hin < 2; ++hin) {
            // a few rows in a row: the state the pieces leave feeds the next step
            Wide p1 = pv, m1 = mv, p2 = pv, m2 = mv;
            for (int row = 0; row < 3; ++row) {
                const WideRow a = wide_step(eq, p1, m1, hin), b = lane_step<W>(eq, p2, m2, hin);
                CHECK(a.pv == b.pv && a.mv == b.mv && a.ph == b.ph && a.mh == b.mh && a.d0 == b.d0);
                p1 = a.pv; m1 = a.mv; p2 = b.pv; m2 = b.mv;
                for (int k = 0; k < N; ++k) eq[k] = (eq[k] << 7) | (eq[k] >> 25);
            }
        }
    }
}

int main() {
    // every (G, P) with G & P == 0 at 10 lanes: 3^10 pairs
    int pairs = 0;
    for (uint64_t G = 0; G < 1024; ++G)
        for (uint64_t P = 0; P < 1024; ++P) {
            if (G & P) continue;
            ++pairs;
            CHECK((rg::edit_carry_mask(G, P) & 1023) == ripple_mask(G, P, 10));
        }
    CHECK(pairs == 59049);
    std::mt19937_64 rng(44);
    for (int it = 0; it < 200000; ++it) {
        uint64_t P = rng(), G = rng();
        if (it % 3 == 0) P |= rng();                 // long runs of propagating lanes
        if (it % 7 == 0) P = ~0ull;
        G &= ~P;
        CHECK(rg::edit_carry_mask(G, P) == ripple_mask(G, P, 64));
    }
    CHECK(rg::edit_carry_mask(1, ~1ull) == ~1ull);       // lane 0 generates, everyone hands it on
    CHECK(rg::edit_carry_mask(0, ~0ull) == 0);
    check_rows<1>(rng);
    check_rows<2>(rng);
    check_rows<4>(rng);
    check_rows<8>(rng);
    return finish("edit bits ok");
}
