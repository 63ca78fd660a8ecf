// TEST TOOL (links the oracle: test infrastructure, never part of the product).
//
// The band of a POA row as the kernels compute it — band_simd (-m 0 SIMD: a closed form in place of the reference's three
// widening loops) and band_plain (scalar -m 0, -m 2), recgraph_amd/csrc/rg_band.hpp compiled for the host — against the
// oracle's set_ampl_for_row (utils.rs:17-98, usize arithmetic), on
//   * every case of a small range: seq_len 1..96, every ms <= me <= seq_len + 2 (and the row-0 case ms = me = 0),
//     r_val 0..seq_len + 10 and -1 (as usize: a row without a path to the sink), bta 0..24;
//   * seeded random cases with seq_len up to 2^20.
// Build with -DRG_BAND_SIMD_LOOPS to check the loop form of band_simd the same way.
//
//   band_check [random cases] [seed]      prints one JSON line; exit status 1 on any difference
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../oracle/orc_common.hpp"
#include "../../recgraph_amd/csrc/rg_band.hpp"

namespace {

struct Counts {
    long long cases = 0, bad_simd = 0, bad_plain = 0;
    std::string first;
};

// one case: row i = 0 when ms = me = 0 (no predecessors), else two predecessors whose best_scoring_pos are ms - 1 and me - 1
void check(Counts& c, size_t ms, size_t me, size_t r_val, size_t seq_len, size_t bta) {
    static std::vector<size_t> preds{0, 1}, bsp(2), none;
    const bool row0 = ms == 0 && me == 0;
    if (!row0) { bsp[0] = ms - 1; bsp[1] = me - 1; }
    const size_t i = row0 ? 0 : 2;
    const auto es = orc::set_ampl_for_row(i, row0 ? none : preds, r_val, bsp, seq_len, bta, true);
    const auto ep = orc::set_ampl_for_row(i, row0 ? none : preds, r_val, bsp, seq_len, bta, false);
    unsigned sl = 0, sr = 0;
    rg::band_simd((int)i, (unsigned)ms, (unsigned)me, (int)r_val, (unsigned)seq_len, (unsigned)bta, sl, sr);
    int pl = 0, pr = 0;
    rg::band_plain(ms, me, (int)r_val, seq_len, bta, pl, pr);
    ++c.cases;
    const bool bs = sl != (unsigned)es.first || sr != (unsigned)es.second;
    const bool bp = pl != (int)ep.first || pr != (int)ep.second;
    c.bad_simd += bs;
    c.bad_plain += bp;
    if ((bs || bp) && c.first.empty()) {
        char b[256];
        snprintf(b, sizeof b, "ms %zu me %zu r %zu seq_len %zu bta %zu: simd %u..%u vs %zu..%zu, plain %d..%d vs %zu..%zu", ms, me, r_val,
                 seq_len, bta, sl, sr, es.first, es.second, pl, pr, ep.first, ep.second);
        c.first = b;
    }
}

}  // namespace

int main(int argc, char** argv) {
    const long long nrandom = argc > 1 ? atoll(argv[1]) : 1000000;
    const unsigned seed = argc > 2 ? (unsigned)atoi(argv[2]) : 1;
    Counts ex, rnd;
    for (size_t n = 1; n <= 96; ++n)
        for (size_t bta = 0; bta <= 24; ++bta)
            for (size_t r = 0; r <= n + 11; ++r) {
                const size_t r_val = r <= n + 10 ? r : SIZE_MAX;     // (and a row that does not reach the sink: -1 as usize)
                check(ex, 0, 0, r_val, n, bta);
                for (size_t ms = 1; ms <= n + 2; ++ms)
                    for (size_t me = ms; me <= n + 2; ++me) check(ex, ms, me, r_val, n, bta);
            }
    std::mt19937_64 rng(seed);
    auto uni = [&](size_t lo, size_t hi) { return lo + (size_t)(rng() % (hi - lo + 1)); };
    for (long long k = 0; k < nrandom; ++k) {
        const size_t n = (size_t)1 << uni(0, 20);
        const size_t seq_len = uni(1, n);
        const size_t ms = k % 16 == 0 ? 0 : uni(1, seq_len);
        const size_t me = ms == 0 ? 0 : (k % 4 == 0 ? ms : uni(ms, seq_len));
        // r-values: distance to the sink in rows, any size; near seq_len on a quarter of the cases (where the band's end moves)
        const size_t r_val = k % 4 == 1 ? (size_t)std::max<long long>(0, (long long)seq_len + (long long)uni(0, 20) - 10) : uni(0, 2 * seq_len + 10);
        const size_t bta = k % 3 == 0 ? uni(0, 40) : uni(0, std::min<size_t>(seq_len, 1u << 16));
        check(rnd, ms, me, r_val, seq_len, bta);
    }
#ifdef RG_BAND_SIMD_LOOPS
    const char* form = "loops";
#else
    const char* form = "closed";
#endif
    printf("{\"band_simd\": \"%s\", \"exhaustive_cases\": %lld, \"exhaustive_bad_simd\": %lld, \"exhaustive_bad_plain\": %lld, "
           "\"random_cases\": %lld, \"random_bad_simd\": %lld, \"random_bad_plain\": %lld, \"first\": \"%s\"}\n",
           form, ex.cases, ex.bad_simd, ex.bad_plain, rnd.cases, rnd.bad_simd, rnd.bad_plain,
           (ex.first.empty() ? rnd.first : ex.first).c_str());
    return ex.bad_simd || ex.bad_plain || rnd.bad_simd || rnd.bad_plain ? 1 : 0;
}
