// The decisions of the pathwise driver (rg_path_driver.hip) as data: which kernels a batch runs, on what geometry, with which
// margins and list sizes.  Plain host arithmetic on (rg_params, graph sizes, longest read, Options, spec_level) — no HIP here, so
// tests/c/plan_check.cpp states the routes without a GPU.  Also the per-graph host tables the driver uploads (rows of every
// path, the 12-mer vote table) and the structs whose sizes the plan counts.
#pragma once
#include <cstddef>
#include <vector>

#include "rg_host.hpp"
#include "layer_window/rg_layer_window.hpp"

namespace rg {

// per-read scalar state carried between the kernels of one batch
struct ReadState {
    uint32_t status;
    int s0;            // best no-recombination score (seed of the search) / m4 best score
    int seed_path;
    int end_row;       // sink row of the chosen path
    int end_row_best;  // semiglobal: row of the overall best last-column value
    int fwd_path, rev_path, fen, rsn, rec_col, displacement;
    float fscore;
    int bound;         // integer lower bound of the final search maximum (>= s0), tightens the pruning
    int sink_val[RG_MAXP];  // A[sink row][n][k]; semiglobal: best last-column value of path k over its rows >= 1
    int trace_score;        // value of the forward layer where the traceback starts (written by k_layer)
    int path_end_row[RG_MAXP];   // semiglobal: first row attaining sink_val[k] (ending_node, pathwise_alignment_recombination.rs:885-897)
};

// one entry of the recombination candidate lists: best member of (row, col) that can still matter
struct Cand {
    int row, col, val, path;
};

// the only HostGraph fields (and the longest read of the batch) the decisions read
struct PathPlanInput {
    int P, L, fslots, rslots, max_path_rows, max_n;
};

struct PathPlan {
    // geometry: columns per lane, waves (column stripes) per read, padded columns, u32 words per (row, group) slot, ints per record
    int C, nwv, wpad, dir_words, recw;
    long long layer_stride, fdirs_stride, rdirs_stride;   // words per read: traceback decisions (2 bits per cell), direction words
    size_t per_read;              // bytes of HBM work buffers per read without the candidate / record lists
    int mode;                     // pipeline selector: the semiglobal modes run the kernels of -m 4 / -m 8 with the `semi` switches
    bool semi;
    int maxmatch;
    bool gaps_nonpos;             // every gap entry <= 0 (then w[.][j] <= (n - j) * max match)
    bool gaps_agree;              // ('-', b) == (b, '-') for every base: the walkers' L key vs the sweep's
    int score_scale;
    bool use16;                   // packed 16-bit rows (rg_sweep16.hip); implies one wave per read
    bool two_sweep, use_rec, spec, pick_two, dsel, spec4, opt16, layer16;
    int layer_window;             // columns of the window the layers are rebuilt in (layer_window/rg_layer_window.hip), 0: full rows
    bool retire, use_split, gather_ok;
    bool retire_fwd, retire_rev;  // `retire` in the forward / reverse sweep of -m 8 (no_retire 3 / 2 keep one of them)
    bool retire4, dsel4;          // -m 4 on its speculative bound: path retirement, direction words of the picked path only
    bool order;                   // longest-first launch order of the sweeps' waves wherever paths retire
    int spec_margin, spec4_margin, dsel_lo, dsel_hi, rec_pen;
    unsigned fcap, rcap, frec_cap, rrec_cap;    // what the lists of a handle start with (regrown on overflow)
    // -m 6 / -m 7 (affine gaps, gap/rg_path_gap.hip): `mode` is RG_MODE_PATHWISE_GAP, `semi` says -m 7; one wave per (read, path),
    // C columns per lane; the direction pass stores gap_words dwords per lane and row (4 bits per cell) for the picked path
    bool gap;
    bool local;                   // -m 12 (gap_local/rg_path_gap_local.hip): the same geometry and buffers, the local kernels
    int gap_words;
    long long gdirs_stride;       // words per read: (rows of the longest path + 1) * gap_words * 64
    // the long family (gap_long/rg_path_gap_long.hip) when the longest read has more than 2047 bases — otherwise the plan IS the
    // base mode's: C = 32, nwv = S = ceil((max_n + 1) / 2048) column stripes walked by ONE wave, gdirs_stride = S * (rows + 1) * 4 * 64,
    // and two boundary buffers (ints per read): 2 * (rows + 1) per path for the score pass, 2 * (rows + 1) for the direction pass
    long long gbnd_stride, gdbnd_stride;
    // the xlong family (gap_xlong/rg_path_gap_xlong.hip) when the longest read has more than 2047 bases — otherwise the plan IS the
    // base mode's: C = 32, nwv = S = ceil((max_n + 1) / 2048) <= 64, gdirs_stride = (rows + 1) * 4 * 64 (ONE stripe), gbnd_stride as
    // above, gdbnd_stride = 0, and (ints per read) (S - 1) * 2 * (rows + 1) of checkpoints; gwalk_bytes: the walk state of a read
    bool gap_xlong;
    long long gckpt_stride;
    size_t gwalk_bytes;
    // the xstrands family (rg_strand_driver.hip): which part of the affine-gap pipeline a job runs (PATH_STAGE_*, plan_gap_stage);
    // PATH_STAGE_ALL in every plan plan_pathwise returns
    int stage;
    // -m 44 / -m 45 (bit-vector edit distance, edit/rg_path_edit.hip): `semi` says -m 45; one wave per (read, path) holds the whole read,
    // edit_words (W = 1, 2, 4, 8: the smallest with max_n <= 2048 W) dwords of 32 columns per lane and bit vector; the direction pass
    // stores 2 W dwords per lane and row (2 bits per cell) for the picked path: gdirs_stride = (rows of the longest path + 1) * 2 W * 64
    // words, the only work buffer beside ReadState.  `gap` stays false: none of the affine-gap kernels but the pick runs
    bool edit;
    int edit_words;
    // -m 94 / -m 95 (edit_xlong/rg_path_edit_xlong.hip) when the longest read has more than 16383 bases — otherwise the plan IS the one
    // of -m 44 / -m 45: edit_words = 8, C = 256, nwv = S = max(2, ceil(max_n / 16384)) <= 8 column stripes walked by ONE wave, gdirs_stride =
    // (rows + 1) * 16 * 64 words (ONE stripe); per (path, stripe but the last) a slot of edit_slot_words u64 that holds two bits per
    // row as two masks per 64 rows (2 * ceil(rows / 64), rounded up to a 128-byte line so that no two waves share one): edit_bnd_stride
    // = P * (S - 1) * edit_slot_words u64 per read; gwalk_bytes: the walk state of a read
    bool edit_xlong;
    int edit_slot_words;
    long long edit_bnd_stride;
    // -m 64 / -m 65 (both strands in one wave, edit_strands/rg_edit_strands.hip): `edit` is set and the direction pass, the walk and
    // gdirs_stride are those of -m 44 / -m 45 at edit_words (the smallest with max_n <= 2048 W); the score pass runs at edit_pair_words
    // (1, 2, 4, 8, 16: the smallest with max_n <= 1024 W, a strand takes 32 lanes).  per_read counts a second ReadState (the reverse
    // strand's picks), the read on the strand that won (edit_orient_bytes: max_n rounded up to 16) and the strand byte
    bool edit_strands;
    int edit_pair_words;
    size_t edit_orient_bytes;

    // ... with candidate lists of fcap / rcap entries and record lists of frec_cap / rrec_cap records
    size_t per_read_all(unsigned fcap_, unsigned rcap_, unsigned frec_cap_, unsigned rrec_cap_) const {
        if (mode != RG_MODE_RECOMBINATION) return per_read;
        return per_read + (size_t)fcap_ * sizeof(Cand) + (size_t)rcap_ * (sizeof(Cand) + 4) +
               (use_rec ? (size_t)(frec_cap_ + rrec_cap_) * recw * 4 : 0);
    }
};

// spec_level: 0 = the batch itself; 1 = the reads whose speculation failed, once more with a generous margin; 2 = what fails
// even that, with the provable bound.  RG_ERR_ARG / RG_ERR_CAPACITY (through fail()) for batches the kernels cannot take.
int plan_pathwise(const rg_params& p, const PathPlanInput& in, const Options& opt, int spec_level, PathPlan& out);
// The plan of the edit-distance modes (what plan_pathwise returns for a mode of rg_edit_modes.hpp), with every refusal of theirs, in the
// words of the mode's family: gap costs other than (0, -1) or an ACGTN x ACGTN entry other than 0 / -1, an amb_mode bit, a read over the
// family's limit (RG_ERR_ARG), mode 16's 2^28 budget (RG_ERR_CAPACITY).  In every family the plan of -m 44 / -m 45 up to 16383 bases, the
// striped one (PathPlan::edit_xlong) beyond.  `out` must be a cleared plan
int plan_pathwise_edit(const rg_params& p, const PathPlanInput& in, PathPlan& out);
// The plan of the both-strands edit-distance modes (rg_edit_strands_modes.hpp; what plan_pathwise returns for -m 64 / -m 65): the
// admission of -m 44 / -m 45 with amb_mode 0 or 4 admitted and every other value refused in the modes' own words (PathPlan::edit_strands)
int plan_pathwise_edit_strands(const rg_params& p, const PathPlanInput& in, PathPlan& out);

// The stages of an affine-gap pipeline (PathJob::stage, rg_path_args.hpp).  PICK: score pass + pick, and the pick goes out into the
// job's records (status, score, path, end row; no ops).  TRACE: the picks come back in from the job's records, then the direction
// pass and the walk as they are.
enum { PATH_STAGE_ALL = 0, PATH_STAGE_PICK = 1, PATH_STAGE_TRACE = 2 };
// Narrows a plan of plan_pathwise to one stage: `stage`, and `per_read` = what the stage's kernels touch.  PICK: ReadState and, when
// striped, the score pass's P * 2 * (rows + 1) boundary ints; TRACE: the whole pipeline's minus those ints.  Geometry, strides and
// kernels are untouched.  RG_ERR_ARG for a plan that is no affine-gap plan, and for the striped plan of the long family, whose
// direction pass has no caller that runs it alone.
int plan_gap_stage(PathPlan& plan, int stage);

bool sweep16_admissible(const DevScores& sc, int max_path_rows, int max_n, int C);

// rows of every path in program order (rows of path k: prow[poff[k] .. poff[k + 1])), with the direction-word slot of the
// group holding the path
void build_path_rows(const HostGraph& h, bool fwd, std::vector<int>& poff, std::vector<int>& prow, std::vector<int>& pslot);
// 12-mers of every path -> paths that contain them (k_pick votes with it): open addressing, 24-bit keys or 0xffffffff; (P + 63) / 64
// words of path bits per entry; keys.size() is a power of two.  poff / prow: the FORWARD lists of build_path_rows.
void build_kmer_table(const HostGraph& h, const std::vector<int>& poff, const std::vector<int>& prow, std::vector<uint32_t>& keys,
                      std::vector<unsigned long long>& masks);

}  // namespace rg
