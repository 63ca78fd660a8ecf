// The two both-strands edit-distance pathwise modes (-m 64 global, -m 65 semiglobal; RG_MODE_PATHWISE_EDIT_STRANDS in
// include/recgraph_hip.h): modes 44 / 45 with both strands of every read scored in ONE wave (edit_strands/rg_edit_strands.hip).
// Deliberately NO row of kEditFamilies (rg_edit_modes.hpp) and none of the affine-gap table: edit_mode(64) and gap_mode(64) stay
// invalid, because the plan (a second ReadState, an oriented read buffer, a strand byte), the word count of the score pass and the
// amb_mode rule (0 or 4; 12 refused) are not those of any row there.  The plan (rg_path_plan.cpp: plan_pathwise_edit_strands),
// rg_batch_create, the stream, the formatter and the strand driver ask edit_strands_mode(); recgraph_amd/_lib.py holds the same
// values as EDIT_STRANDS_*.
#pragma once
#include "rg_edit_modes.hpp"

namespace rg {

// a strand takes half a wave: 32 lanes of 32 W bits, W <= 16 (W = 16: the 16383 bases of modes 44 / 45 at W = 8 over all 64 lanes)
constexpr int EDIT_STRANDS_MAX_WORDS = 16;
constexpr int EDIT_STRANDS_MAX_READ = EDIT_MAX_READ;      // 16383 bases

constexpr const char* kEditStrandsScoreRefusal =
    "the both-strands edit-distance pathwise modes (-m 64 / -m 65) take unit costs only: gap_open 0, gap_ext -1 and every ACGTN x ACGTN "
    "score 0 or -1 (-M 0 -X 1 -O 0 -E 1, or a 0 / -1 matrix); every other scoring is what -m 26 / -m 27 are for";
constexpr const char* kEditStrandsAmbRefusal =
    "amb_mode must be 0 or 4 in the both-strands edit-distance pathwise modes (-m 64 / -m 65): both strands of every read are scored in "
    "one pass, so a 12-mer vote (amb_mode 12) would save nothing and would change the rule";
constexpr const char* kEditStrandsLenRefusal =
    "reads longer than 16383 bases are not supported by the both-strands edit-distance pathwise modes (-m 64 / -m 65)";

struct EditStrandsMode {
    bool valid;                   // false: neither of the two modes — then `semi` is false
    bool semi;                    // the rule of mode 7 (otherwise: of mode 6)
};
constexpr EditStrandsMode edit_strands_mode(int mode) {
    return EditStrandsMode{mode == RG_MODE_PATHWISE_EDIT_STRANDS || mode == RG_MODE_PATHWISE_EDIT_SEMI_STRANDS, mode == RG_MODE_PATHWISE_EDIT_SEMI_STRANDS};
}
// the mode whose record and line `mode` has: 6 or 7 for the two modes here and for an edit-distance mode, `mode` itself otherwise
constexpr int edit_any_base_mode(int mode) {
    return !edit_strands_mode(mode).valid ? edit_base_mode(mode) : edit_strands_mode(mode).semi ? RG_MODE_PATHWISE_GAP_SEMI : RG_MODE_PATHWISE_GAP;
}

static_assert(RG_MODE_PATHWISE_EDIT_STRANDS == RG_MODE_PATHWISE_EDIT + 20 && RG_MODE_PATHWISE_EDIT_SEMI_STRANDS == RG_MODE_PATHWISE_EDIT_SEMI + 20 &&
                  32 * EDIT_STRANDS_MAX_WORDS * (WAVE / 2) == EDIT_STRANDS_MAX_READ + 1,
              "numbered `mode + 20` as the strands family of the affine-gap modes is; half a wave's bits at W = 16");
static_assert(!edit_mode(RG_MODE_PATHWISE_EDIT_STRANDS).valid && !gap_mode(RG_MODE_PATHWISE_EDIT_STRANDS).valid &&
                  !edit_mode(RG_MODE_PATHWISE_EDIT_SEMI_STRANDS).valid && !gap_mode(RG_MODE_PATHWISE_EDIT_SEMI_STRANDS).valid,
              "the two modes are rows of neither table");

}  // namespace rg
