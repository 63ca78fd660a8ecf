// The mode table (recgraph_amd/csrc/rg_gap_modes.hpp) as the affine-gap plan checks ask it.
#pragma once
#include <initializer_list>

#include "plan_check_common.hpp"

namespace gap_check {
// is `mode` a member of family `f`; the mode of `mode`'s rule in family `f`;
// does `mode` have the long family's read limit (the long family and the one that runs its passes on both strands); every mode of
// the given families, family by family
[[maybe_unused]] static bool is_family(int mode, int f) { return gap_mode(mode).valid && gap_mode(mode).family == &kGapFamilies[f]; }
[[maybe_unused]] static int in_family(int mode, int f) { return path_gap_base_mode(mode) + kGapFamilies[f].offset; }
[[maybe_unused]] static bool long_limit(int mode) { return gap_mode(mode).valid && gap_mode(mode).family->max_stripes == GAP_LONG_MAX_STRIPES; }
[[maybe_unused]] static std::vector<int> family_modes(std::initializer_list<int> fams) {
    std::vector<int> out;
    for (int f : fams)
        for (int base : kGapRuleBase) out.push_back(base + kGapFamilies[f].offset);
    return out;
}
}  // namespace gap_check
