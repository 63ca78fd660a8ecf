// What an affine-gap pathwise mode IS: a rule (global 6, semiglobal 7, local 12) in a family (how long a read may be, which strands,
// which traceback), `mode = rule's base + family's offset`.  ONE table; the plan (rg_path_plan.cpp), rg_batch_create, the stream, the
// formatter and the strand driver ask gap_mode() and read the row.  recgraph_amd/_lib.py holds the same rows for the Python side, and
// DESIGN 4.8 the table in words.  A new family is a row here, a row there, and its three #defines in include/recgraph_hip.h.
#pragma once
#include "rg_codes.hpp"

#include "../../include/recgraph_hip.h"

namespace rg {

// column stripes of 32 * WAVE = 2048 columns one wave walks per read: the cap of gap_long/ (a.S of its launchers) and the one the plan
// of gap_xlong/ lifts it to; the longest read of a family is its stripes * 2048 - 1 bases
constexpr int GAP_LONG_MAX_STRIPES = 8;               // 16383 bases
constexpr int GAP_XLONG_MAX_STRIPES = 64;             // 131071 bases

enum GapRule { GAP_RULE_GLOBAL = 0, GAP_RULE_SEMI = 1, GAP_RULE_LOCAL = 2 };
constexpr int kGapRuleBase[3] = {RG_MODE_PATHWISE_GAP, RG_MODE_PATHWISE_GAP_SEMI, RG_MODE_PATHWISE_GAP_LOCAL};

struct GapFamily {
    int offset;                   // mode - base mode
    int max_stripes;              // longest read: max_stripes * 32 * WAVE - 1 bases
    bool both_strands;            // the handle always sets RG_AMB_BOTH_STRANDS; amb_mode 0, 4 or (global, semiglobal) 12, otherwise 0 alone
    bool one_stripe_dirs;         // striped reads keep ONE stripe of direction words: the checkpointed traceback of gap_xlong/
    bool staged;                  // two PICK stages and one TRACE stage (rg_strand_driver.hip): no second op area, no merge
    // the plan's refusals of an amb_mode and of a read that is too long; *_local: what the local rule says instead, where it differs
    const char* amb_refusal;
    const char* len_refusal;
    const char* amb_refusal_local;
    const char* len_refusal_local;
    constexpr int max_read() const { return max_stripes * 32 * WAVE - 1; }
    const char* amb_text(bool local) const { return local && amb_refusal_local ? amb_refusal_local : amb_refusal; }
    const char* len_text(bool local) const { return local && len_refusal_local ? len_refusal_local : len_refusal; }
};
enum { GAP_FAM_BASE, GAP_FAM_LONG, GAP_FAM_STRANDS, GAP_FAM_XLONG, GAP_FAM_XSTRANDS, GAP_FAMILIES };
inline constexpr GapFamily kGapFamilies[GAP_FAMILIES] = {
    // one wave keeps H and Y of the current row in registers, up to 32 columns per lane: the reads as given
    {0, 1, false, false, false,
     "amb_mode must be 0 in the affine-gap pathwise modes (-m 6 / -m 7): they align the reads as given",
     "reads longer than 2047 bases are not supported by the affine-gap pathwise modes (-m 6 / -m 7)",
     "amb_mode must be 0 in the local affine-gap pathwise mode (-m 12): it aligns the reads as given",
     "reads longer than 2047 bases are not supported by the local affine-gap pathwise mode (-m 12)"},
    // the same rule, record and line for reads walked in column stripes (gap_long/)
    {10, GAP_LONG_MAX_STRIPES, false, false, false,
     "amb_mode must be 0 in the long-read affine-gap pathwise modes (-m 16 / -m 17 / -m 22): they align the reads as given",
     "reads longer than 16383 bases are not supported by the long-read affine-gap pathwise modes (-m 16 / -m 17 / -m 22, and -m 26 / -m 27 / -m 32 on both strands)",
     nullptr, nullptr},
    // ... on both strands: two passes, each one of the long family's (gap_strands/)
    {20, GAP_LONG_MAX_STRIPES, true, false, false,
     "amb_mode must be 0, 4 or 12 in the both-strands affine-gap pathwise modes (-m 26 / -m 27), 0 or 4 in -m 32",
     "reads longer than 16383 bases are not supported by the long-read affine-gap pathwise modes (-m 16 / -m 17 / -m 22, and -m 26 / -m 27 / -m 32 on both strands)",
     nullptr, nullptr},
    // the long family's rule and bytes once more, with a traceback that keeps one stripe of direction words (gap_xlong/)
    {50, GAP_XLONG_MAX_STRIPES, false, true, false,
     "amb_mode must be 0 in the affine-gap pathwise modes for reads of up to 131071 bases (-m 56 / -m 57 / -m 62): they align the reads as given",
     "reads longer than 131071 bases are not supported by the affine-gap pathwise modes -m 56 / -m 57 / -m 62",
     nullptr, nullptr},
    // ... on both strands: the strand rule of the strands family on the PICKED scores of the xlong pipeline, the traceback run once
    // per read, on the strand that won (gap_xstrands/)
    {70, GAP_XLONG_MAX_STRIPES, true, true, true,
     "amb_mode must be 0, 4 or 12 in the both-strands affine-gap pathwise modes for reads of up to 131071 bases (-m 76 / -m 77), 0 or 4 in -m 82",
     "reads longer than 131071 bases are not supported by the both-strands affine-gap pathwise modes -m 76 / -m 77 / -m 82",
     nullptr, nullptr},
};

struct GapMode {
    bool valid;                   // false: no affine-gap pathwise mode — then `rule` is GAP_RULE_GLOBAL and `family` the base row, whose flags are all off
    GapRule rule;
    const GapFamily* family;
};
constexpr GapMode gap_mode(int mode) {
    for (const GapFamily& f : kGapFamilies)
        for (int r = 0; r < 3; ++r)
            if (mode == kGapRuleBase[r] + f.offset) return GapMode{true, (GapRule)r, &f};
    return GapMode{false, GAP_RULE_GLOBAL, &kGapFamilies[GAP_FAM_BASE]};
}
// the mode whose rule, record and line `mode` has: 6, 7 or 12 for an affine-gap pathwise mode, `mode` itself otherwise
constexpr int path_gap_base_mode(int mode) { return gap_mode(mode).valid ? kGapRuleBase[gap_mode(mode).rule] : mode; }

#define RG_GAP_FAMILY_DEFINES(suffix, fam)                                                                            \
    static_assert(RG_MODE_PATHWISE_GAP##suffix == kGapRuleBase[GAP_RULE_GLOBAL] + kGapFamilies[fam].offset &&         \
                      RG_MODE_PATHWISE_GAP_SEMI##suffix == kGapRuleBase[GAP_RULE_SEMI] + kGapFamilies[fam].offset &&  \
                      RG_MODE_PATHWISE_GAP_LOCAL##suffix == kGapRuleBase[GAP_RULE_LOCAL] + kGapFamilies[fam].offset,  \
                  "include/recgraph_hip.h and the family table disagree")
RG_GAP_FAMILY_DEFINES(, GAP_FAM_BASE);
RG_GAP_FAMILY_DEFINES(_LONG, GAP_FAM_LONG);
RG_GAP_FAMILY_DEFINES(_STRANDS, GAP_FAM_STRANDS);
RG_GAP_FAMILY_DEFINES(_XLONG, GAP_FAM_XLONG);
RG_GAP_FAMILY_DEFINES(_XSTRANDS, GAP_FAM_XSTRANDS);
#undef RG_GAP_FAMILY_DEFINES

}  // namespace rg
