// What a bit-vector edit-distance pathwise mode IS: a rule (global 44, semiglobal 45) in a family (how long a read may be), `mode = rule's
// base + family's offset`; each family is a family of the affine-gap table (rg_gap_modes.hpp) restricted to unit costs: its rule, bytes
// and read limit.  ONE table; the plan (rg_path_plan.cpp: plan_pathwise_edit), rg_batch_create, the stream and the formatter ask
// edit_mode() and read the row.  recgraph_amd/_lib.py holds the same rows for the Python side, and DESIGN 4.14 the table in words.  A new
// family is a row here, a row there, and its two #defines in include/recgraph_hip.h.  The modes are NO rows of the affine-gap table
// (gap_mode(44) stays invalid): its plan, record sizes and amb_mode rules are not theirs.
#pragma once
#include "rg_gap_modes.hpp"

namespace rg {

// one wave holds the whole read: 64 lanes of 32 W bits, W <= 8 (edit/rg_path_edit.hip)
constexpr int EDIT_MAX_WORDS = 8;
constexpr int EDIT_MAX_READ = 32 * EDIT_MAX_WORDS * WAVE - 1;      // 16383 bases
// ... or a column stripe of the read, one wave's 16384 bits (edit_xlong/rg_path_edit_xlong.hip).  A batch whose longest read fits one
// wave is planned and run as one of the base family, whatever its family
constexpr int EDIT_XLONG_STRIPE = 32 * EDIT_MAX_WORDS * WAVE;      // 16384 columns: bit t of stripe s is column 16384 s + t + 1
constexpr int EDIT_XLONG_MAX_STRIPES = 8;
constexpr int EDIT_XLONG_MAX_READ = EDIT_XLONG_MAX_STRIPES * EDIT_XLONG_STRIPE - 1;      // 131071 bases

constexpr int kEditRuleBase[2] = {RG_MODE_PATHWISE_EDIT, RG_MODE_PATHWISE_EDIT_SEMI};      // global, semiglobal

struct EditFamily {
    int offset;                   // mode - base mode
    int max_read;                 // longest read, in bases
    int gap_family;               // the row of kGapFamilies whose rule, bytes and read limit these are, at unit costs
    // the plan's refusals of a scoring that is not unit costs, of an amb_mode and of a read that is too long
    const char* score_refusal;
    const char* amb_refusal;
    const char* len_refusal;
};
enum { EDIT_FAM_BASE, EDIT_FAM_XLONG, EDIT_FAMILIES };
inline constexpr EditFamily kEditFamilies[EDIT_FAMILIES] = {
    {0, EDIT_MAX_READ, GAP_FAM_LONG,
     "the edit-distance pathwise modes (-m 44 / -m 45) take unit costs only: gap_open 0, gap_ext -1 and every ACGTN x ACGTN score 0 or -1 "
     "(-M 0 -X 1 -O 0 -E 1, or a 0 / -1 matrix); every other scoring is what -m 16 / -m 17 are for",
     "amb_mode must be 0 in the edit-distance pathwise modes (-m 44 / -m 45): they align the reads as given",
     "reads longer than 16383 bases are not supported by the edit-distance pathwise modes (-m 44 / -m 45)"},
    {50, EDIT_XLONG_MAX_READ, GAP_FAM_XLONG,
     "the edit-distance pathwise modes (-m 94 / -m 95) take unit costs only: gap_open 0, gap_ext -1 and every ACGTN x ACGTN score 0 or -1 "
     "(-M 0 -X 1 -O 0 -E 1, or a 0 / -1 matrix); every other scoring is what -m 56 / -m 57 are for",
     "amb_mode must be 0 in the edit-distance pathwise modes (-m 94 / -m 95): they align the reads as given",
     "reads longer than 131071 bases are not supported by the edit-distance pathwise modes (-m 94 / -m 95)"},
};

struct EditMode {
    bool valid;                   // false: no edit-distance mode — then `semi` is false and `family` the base row
    bool semi;                    // the rule of mode 7 (otherwise: of mode 6)
    const EditFamily* family;
};
constexpr EditMode edit_mode(int mode) {
    for (const EditFamily& f : kEditFamilies)
        for (int r = 0; r < 2; ++r)
            if (mode == kEditRuleBase[r] + f.offset) return EditMode{true, r == 1, &f};
    return EditMode{false, false, &kEditFamilies[EDIT_FAM_BASE]};
}
// the mode whose record and line `mode` has: 6 or 7 for an edit-distance mode (the base modes of its gap family), `mode` itself otherwise
constexpr int edit_base_mode(int mode) {
    return !edit_mode(mode).valid ? mode : edit_mode(mode).semi ? RG_MODE_PATHWISE_GAP_SEMI : RG_MODE_PATHWISE_GAP;
}

// a family's two #defines are its rules' bases plus its offset, and its read limit is the one of its gap family
constexpr bool edit_family_is(int fam, int global, int semi) {
    const EditFamily& f = kEditFamilies[fam];
    return global == kEditRuleBase[0] + f.offset && semi == kEditRuleBase[1] + f.offset && f.max_read == kGapFamilies[f.gap_family].max_read();
}
static_assert(edit_family_is(EDIT_FAM_BASE, RG_MODE_PATHWISE_EDIT, RG_MODE_PATHWISE_EDIT_SEMI) &&
                  edit_family_is(EDIT_FAM_XLONG, RG_MODE_PATHWISE_EDIT_XLONG, RG_MODE_PATHWISE_EDIT_SEMI_XLONG),
              "include/recgraph_hip.h, the gap family table and the edit family table disagree");
static_assert(RG_MODE_PATHWISE_EDIT == 44 && RG_MODE_PATHWISE_EDIT_SEMI == 45 && EDIT_MAX_READ == 16383 && EDIT_XLONG_MAX_READ == 131071,
              "the rules' bases, one wave's bits and eight stripes of them");

}  // namespace rg
