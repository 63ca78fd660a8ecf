// CPU check of recgraph_amd/csrc/edit_strands/rg_edit_pair_bits.hpp, the two cross-lane pieces of the half-wave row step of
// k_edit_score_pair (-m 64 / -m 65), together with the per-chunk pieces of edit/rg_edit_bits.hpp, with the very functions the kernel calls:
// the pair carry mask against two bit-serial ripples of 32 lanes, and the row step over 64 host "lanes" of W = 1, 2, 16 words — the
// ballots and the lane shifts done by hand, the shift wave-wide and then overridden as the kernel does — against TWO independent plain row
// steps on wide integers of 32 * 32 W bits, one per half.  Cases: random Eq / Pv / Mv; the lower half all ones, so that a carry tries
// to leave lane 31; the top bit of lane 31's Ph / Mh set, so that a wave-wide shift would hand it to lane 32.  A stand-alone main, built
// twice by tests/test_pathwise_edit_strands_cpu.py: plain, and with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "edit_strands/rg_edit_pair_bits.hpp"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { ++failures; fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); } \
    } while (0)

typedef std::vector<uint32_t> Wide;      // word 0 the lowest

static uint32_t ripple_mask32(uint32_t G, uint32_t P) {
    uint32_t m = 0, c = 0;
    for (int l = 0; l < 32; ++l) {
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

struct WideRow { Wide pv, mv, ph, mh, d0; };
// the row step as edit/rg_edit_bits.hpp's comment writes it, on one whole vector
static WideRow wide_step(const Wide& eq, const Wide& pv, const Wide& mv, uint32_t hin) {
    const size_t n = eq.size();
    Wide a(n), xv(n), xh(n);
    for (size_t k = 0; k < n; ++k) { a[k] = eq[k] & pv[k]; xv[k] = eq[k] | mv[k]; }
    const Wide sum = w_add(a, pv);
    WideRow r;
    r.ph.resize(n); r.mh.resize(n); r.d0.resize(n); r.pv.resize(n); r.mv.resize(n);
    for (size_t k = 0; k < n; ++k) {
        xh[k] = (sum[k] ^ pv[k]) | eq[k];
        r.ph[k] = mv[k] | ~(xh[k] | pv[k]);
        r.mh[k] = pv[k] & xh[k];
        r.d0[k] = xh[k] | mv[k];
    }
    const Wide phs = w_shl1(r.ph, hin), mhs = w_shl1(r.mh, 0);
    for (size_t k = 0; k < n; ++k) {
        r.pv[k] = mhs[k] | ~(xv[k] | phs[k]);
        r.mv[k] = phs[k] & xv[k];
    }
    return r;
}

static Wide half_of(const Wide& v, int half) { return Wide(v.begin() + half * (v.size() / 2), v.begin() + (half + 1) * (v.size() / 2)); }
static bool halves_are(const Wide& whole, const Wide& lo, const Wide& hi) { return half_of(whole, 0) == lo && half_of(whole, 1) == hi; }

// the same step as k_edit_score_pair takes it: 64 lanes of W words, two strands of 32 lanes
template <int W>
static WideRow lane_step(const Wide& eq, const Wide& pv, const Wide& mv, uint32_t hin) {
    constexpr int L = 64;
    static uint32_t e[L][W], p[L][W], m[L][W], sum[L][W], ph[L][W], mh[L][W], d0[L][W];
    uint64_t G = 0, P = 0;
    for (int l = 0; l < L; ++l) {
        for (int k = 0; k < W; ++k) { e[l][k] = eq[l * W + k]; p[l][k] = pv[l * W + k]; m[l][k] = mv[l * W + k]; }
        const uint32_t g = rg::edit_sum<W>(e[l], p[l], sum[l]);
        const bool ones = rg::edit_chunk_all_ones<W>(sum[l]);
        CHECK(!(g && ones));
        G |= (uint64_t)g << l;
        P |= (uint64_t)(ones ? 1 : 0) << l;
    }
    const uint64_t cm = rg::edit_pair_carry_mask(G, P);
    for (int l = 0; l < L; ++l) rg::edit_deltas<W>(e[l], p[l], m[l], sum[l], (uint32_t)(cm >> l) & 1u, ph[l], mh[l], d0[l]);
    WideRow r;
    r.pv.resize(L * W); r.mv.resize(L * W); r.ph.resize(L * W); r.mh.resize(L * W); r.d0.resize(L * W);
    uint32_t pin[L], nin[L];
    for (int l = 0; l < L; ++l) {
        // the wave-wide shift by one lane (lane 0 keeps the fill), then the override of the first lane of either half
        pin[l] = rg::edit_pair_shift_in(l == 0 ? hin : ph[l - 1][W - 1] >> 31, l, hin);
        nin[l] = rg::edit_pair_shift_in(l == 0 ? 0u : mh[l - 1][W - 1] >> 31, l, 0u);
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
    constexpr int N = 64 * W, H = 32 * W;
    int leaks = 0;      // cases in which a wave-wide step WOULD differ from the two halves: the cases below must produce some
    for (int it = 0; it < 200; ++it) {
        Wide eq(N), pv(N), mv(N);
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
        if (it % 8 == 1) {
            // the lower half all ones: Eq & Pv + Pv carries out of lane 31; the upper half random
            for (int k = 0; k < H; ++k) { eq[k] = ~0u; pv[k] = ~0u; mv[k] = 0u; }
        }
        if (it % 8 == 2) {
            // lane 31's top bit of Ph set: Mv's top bit set there (Ph = Mv | ...), so the last column of the lower half goes up
            pv[H - 1] &= ~(1u << 31); mv[H - 1] |= 1u << 31;
        }
        if (it % 8 == 3) {
            // lane 31's top bit of Mh set: Pv's top bit and Eq's top bit set there (Mh = Pv & Xh, Xh >= Eq)
            pv[H - 1] |= 1u << 31; mv[H - 1] &= ~(1u << 31); eq[H - 1] |= 1u << 31;
        }
        if (it % 8 == 4) {
            // poly-A against a path without A: nothing matches, Pv all ones (row 0): every column goes up, lane 31's Ph top bit included
            for (int k = 0; k < N; ++k) { eq[k] = 0u; pv[k] = ~0u; mv[k] = 0u; }
        }
        for (uint32_t hin = 0; hin < 2; ++hin) {
            Wide pl = half_of(pv, 0), ml = half_of(mv, 0), pu = half_of(pv, 1), mu = half_of(mv, 1), p2 = pv, m2 = mv;
            for (int row = 0; row < 3; ++row) {
                const WideRow lo = wide_step(half_of(eq, 0), pl, ml, hin), hi = wide_step(half_of(eq, 1), pu, mu, hin);
                const WideRow whole = wide_step(eq, p2, m2, hin);      // what a wave-wide step would give: NOT the expectation
                const WideRow b = lane_step<W>(eq, p2, m2, hin);
                CHECK(halves_are(b.pv, lo.pv, hi.pv) && halves_are(b.mv, lo.mv, hi.mv));
                CHECK(halves_are(b.ph, lo.ph, hi.ph) && halves_are(b.mh, lo.mh, hi.mh) && halves_are(b.d0, lo.d0, hi.d0));
                if (!halves_are(whole.pv, lo.pv, hi.pv) || !halves_are(whole.mv, lo.mv, hi.mv)) ++leaks;
                pl = lo.pv; ml = lo.mv; pu = hi.pv; mu = hi.mv; p2 = b.pv; m2 = b.mv;
                for (int k = 0; k < N; ++k) eq[k] = (eq[k] << 7) | (eq[k] >> 25);
            }
        }
    }
    CHECK(leaks >= 100);
}

int main() {
    // every (G, P) with G & P == 0 at 8 lanes around the seam: lanes 28 .. 35
    for (uint64_t G = 0; G < 256; ++G)
        for (uint64_t P = 0; P < 256; ++P) {
            if (G & P) continue;
            const uint64_t g = G << 28, p = P << 28;
            const uint64_t want = (uint64_t)ripple_mask32((uint32_t)g, (uint32_t)p) | ((uint64_t)ripple_mask32((uint32_t)(g >> 32), (uint32_t)(p >> 32)) << 32);
            CHECK(rg::edit_pair_carry_mask(g, p) == want);
        }
    std::mt19937_64 rng(64);
    for (int it = 0; it < 200000; ++it) {
        uint64_t P = rng(), G = rng();
        if (it % 3 == 0) P |= rng();                 // long runs of propagating lanes
        if (it % 7 == 0) P = ~0ull;
        G &= ~P;
        const uint64_t want = (uint64_t)ripple_mask32((uint32_t)G, (uint32_t)P) | ((uint64_t)ripple_mask32((uint32_t)(G >> 32), (uint32_t)(P >> 32)) << 32);
        CHECK(rg::edit_pair_carry_mask(G, P) == want);
    }
    // lane 0 generates and everyone hands it on: the carry stops at lane 31, lane 32 takes none
    CHECK(rg::edit_pair_carry_mask(1, ~1ull) == 0xfffffffeull);
    CHECK(rg::edit_pair_carry_mask(1ull | (1ull << 32), ~(1ull | (1ull << 32))) == 0xfffffffefffffffeull);
    CHECK(rg::edit_pair_carry_mask(1ull << 31, 0) == 0);
    CHECK(rg::edit_pair_shift_in(1, 0, 0) == 0 && rg::edit_pair_shift_in(1, 32, 0) == 0 && rg::edit_pair_shift_in(0, 32, 1) == 1);
    CHECK(rg::edit_pair_shift_in(1, 31, 0) == 1 && rg::edit_pair_shift_in(1, 33, 0) == 1 && rg::edit_pair_shift_in(0, 1, 1) == 0);
    check_rows<1>(rng);
    check_rows<2>(rng);
    check_rows<16>(rng);
    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    puts("edit pair bits ok");
    return 0;
}
