// The bit-vector edit-distance pathwise modes (-m 44 global, -m 45 semiglobal; RG_MODE_PATHWISE_EDIT in include/recgraph_hip.h): the
// rules of modes 16 and 17 restricted to unit costs, computed by the kernels of edit/rg_path_edit.hip.  They are NO rows of the
// affine-gap family table (rg_gap_modes.hpp: gap_mode(44) stays invalid): no family, no strands, one read limit.  The plan
// (rg_path_plan.cpp: plan_pathwise_edit), rg_batch_create, the stream and the formatter ask edit_mode().  recgraph_amd/_lib.py holds
// the same two constants for the Python side, and the two of modes 94 / 95 (edit_xlong_mode, below).
#pragma once
#include "rg_codes.hpp"

#include "../../include/recgraph_hip.h"

namespace rg {

// one wave holds the whole read: 64 lanes of 32 W bits, W <= 8
constexpr int EDIT_MAX_WORDS = 8;
constexpr int EDIT_MAX_READ = 32 * EDIT_MAX_WORDS * WAVE - 1;      // 16383 bases: the limit of modes 16 and 17

struct EditMode {
    bool valid;                   // false: no edit-distance mode, and `semi` is false
    bool semi;                    // -m 45: the rule of mode 17 (mode 44: of mode 16)
};
constexpr EditMode edit_mode(int mode) {
    return mode == RG_MODE_PATHWISE_EDIT ? EditMode{true, false} : mode == RG_MODE_PATHWISE_EDIT_SEMI ? EditMode{true, true} : EditMode{false, false};
}
// -m 94 / -m 95 (RG_MODE_PATHWISE_EDIT_XLONG in include/recgraph_hip.h): the same two rules for reads of up to 131071 bases, in column
// stripes of one wave's 16384 bits (edit_xlong/rg_path_edit_xlong.hip).  A lookup of their own: edit_mode(94) stays invalid, as
// gap_mode(44) does.  A batch of theirs whose longest read fits one wave is planned and run as mode 44 / 45
constexpr int EDIT_XLONG_STRIPE = 32 * EDIT_MAX_WORDS * WAVE;      // 16384 columns: bit t of stripe s is column 16384 s + t + 1
constexpr int EDIT_XLONG_MAX_STRIPES = 8;
constexpr int EDIT_XLONG_MAX_READ = EDIT_XLONG_MAX_STRIPES * EDIT_XLONG_STRIPE - 1;      // 131071 bases: the limit of modes 56 and 57
constexpr EditMode edit_xlong_mode(int mode) {
    return mode == RG_MODE_PATHWISE_EDIT_XLONG ? EditMode{true, false} : mode == RG_MODE_PATHWISE_EDIT_SEMI_XLONG ? EditMode{true, true} : EditMode{false, false};
}
// either lookup
constexpr EditMode edit_any_mode(int mode) { return edit_mode(mode).valid ? edit_mode(mode) : edit_xlong_mode(mode); }

// the mode whose record and line `mode` has: 6 or 7 for an edit-distance mode (the base modes of 16 / 17 and 56 / 57), `mode` itself otherwise
constexpr int edit_base_mode(int mode) {
    return !edit_any_mode(mode).valid ? mode : edit_any_mode(mode).semi ? RG_MODE_PATHWISE_GAP_SEMI : RG_MODE_PATHWISE_GAP;
}

static_assert(RG_MODE_PATHWISE_EDIT == 44 && RG_MODE_PATHWISE_EDIT_SEMI == 45, "include/recgraph_hip.h and rg_edit_modes.hpp disagree");
static_assert(RG_MODE_PATHWISE_EDIT_XLONG == RG_MODE_PATHWISE_EDIT + 50 && RG_MODE_PATHWISE_EDIT_SEMI_XLONG == RG_MODE_PATHWISE_EDIT_SEMI + 50,
              "include/recgraph_hip.h and rg_edit_modes.hpp disagree");
static_assert(EDIT_MAX_READ == 16383, "the read limit of modes 44 and 45 is the one of modes 16 and 17");
static_assert(EDIT_XLONG_MAX_READ == 131071, "the read limit of modes 94 and 95 is the one of modes 56 and 57");

}  // namespace rg
