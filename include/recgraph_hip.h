/*
 * recgraph_hip.h — C ABI of the MI355X-native RecGraph DP hot path.
 *
 * Drop-in boundary for the reference's per-read alignment calls.  Every entry point names the
 * reference interface it replaces (file:line relative to the RecGraph source tree).  Plain
 * pointers and sizes only; no C++/torch types cross this boundary.  All functions return
 * RG_OK (0) or a negative rg_status; none of them aborts (the reference panics instead).
 *
 * Thread-safety: a graph handle is immutable after creation and may be shared by threads and by
 * devices (its device tables are uploaded once per HIP device, under a lock, by the first batch
 * created on that device); a batch handle is bound to the device that was current when it was
 * created (every call on it selects that device) and must be used by one thread at a time.
 */
#ifndef RECGRAPH_HIP_H
#define RECGRAPH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum rg_status {
    RG_OK = 0,
    RG_ERR_ARG = -1,         /* bad argument (null pointer, unsupported mode, empty read ...) */
    RG_ERR_GFA = -2,         /* GFA text not usable (non-numeric names, '-' orientations ...)  */
    RG_ERR_NO_DEVICE = -3,   /* no HIP device / HIP runtime error: the product never falls back to CPU */
    RG_ERR_GRAPH = -4,       /* graph violates a precondition of the reference (not topological, >256 paths ...) */
    RG_ERR_CAPACITY = -5,    /* internal work buffer exhausted even after regrowth */
    RG_ERR_HIP = -6
} rg_status;

/* per-read status bits (rg_result_status) */
#define RG_READ_OK 0u
#define RG_READ_BAND_WARNING 1u     /* reference prints "Band length probably too short, ..." (global_abpoa.rs:406-409, gap_global_abpoa.rs:225-227) */
#define RG_READ_BAND_NOT_ENOUGH 2u  /* reference prints "band not enough for correct output" and an empty GAF (gaf_output.rs:861-864) */
#define RG_READ_WOULD_PANIC 4u      /* reference would panic on this read (index out of range, set_path_cell('u') ...) */
#define RG_READ_BAD_BASE 8u         /* read contains a character outside ACGTN (reference: HashMap unwrap panic) */
#define RG_READ_UNALIGNED 16u       /* RG_MODE_PATHWISE_GAP_LOCAL only: the read has no local alignment (best score 0); no record, no text */

/* Alignment modes: the `-m` values of the reference CLI (args_parser.rs:31-38) on the hot path. */
#define RG_MODE_GLOBAL_POA 0        /* global_abpoa::exec_simd          src/global_abpoa.rs:10      */
#define RG_MODE_GLOBAL_POA_SCALAR 10/* global_abpoa::exec (no-AVX2 path) src/global_abpoa.rs:260     */
#define RG_MODE_GAP_POA 2           /* gap_global_abpoa::exec           src/gap_global_abpoa.rs:11  */
#define RG_MODE_PATHWISE 4          /* pathwise_alignment::exec         src/pathwise_alignment.rs:5 */
#define RG_MODE_RECOMBINATION 8     /* pathwise_alignment_recombination::exec (aln_mode 8) src/pathwise_alignment_recombination.rs:23 */
#define RG_MODE_PATHWISE_SEMI 5     /* pathwise_alignment_semiglobal::exec  src/pathwise_alignment_semiglobal.rs:6 */
#define RG_MODE_RECOMBINATION_SEMI 9/* pathwise_alignment_recombination::exec (aln_mode 9) */
#define RG_MODE_LOCAL_POA 1         /* local_poa::exec_simd             src/local_poa.rs:9          */
#define RG_MODE_LOCAL_POA_SCALAR 11 /* local_poa::exec (no-AVX2 path)   src/local_poa.rs:176        */
#define RG_MODE_GAP_LOCAL_POA 3     /* gap_local_poa::exec              src/gap_local_poa.rs:6      */
/*
 * RG_MODE_PATHWISE_GAP (6, global) and RG_MODE_PATHWISE_GAP_SEMI (7, semiglobal): pathwise alignment with affine gaps.
 * The reference lists both as EXPERIMENTAL (README.md:62), prints only "Best path sequence i: k" for them (main.rs:271-288)
 * and its pathwise_alignment_gap.rs disagrees with itself (:338), so there is nothing to be byte-identical to.  The two
 * modes therefore have A DEFINITION OF THEIR OWN, and they return a GAF record in the -m 4 format:
 *   INPUTS.  For path k, b_1..b_m are the bases of its rows in path order (without row 0 and without 'F'); s_1..s_n is the
 *     read after the usual canonicalisation; o = gap_open <= 0, e = gap_ext <= 0, a gap of length g costs o + g * e
 *     (pathwise_alignment_gap.rs:28,45); sc(a, b) = scores[a * 6 + b] (the '-' entries are not read, as in -m 2).  i32
 *     arithmetic; NEG is a sentinel that can never win.
 *   RECURRENCE, independently for every path (exact Gotoh per path, not the alpha-follows-member coding of -m 4):
 *     H[0][0] = 0
 *     X[0][j] = o + e * j,  H[0][j] = X[0][j],  Y[0][j] = NEG                        (j >= 1)
 *     -m 6:  Y[i][0] = o + e * i,  H[i][0] = Y[i][0],  X[i][0] = NEG                 (i >= 1)
 *     -m 7:  H[i][0] = 0,  Y[i][0] = X[i][0] = NEG                                   (i >= 1: the path may start anywhere)
 *     Y[i][j] = max(H[i-1][j] + o + e, Y[i-1][j] + e)                                (consumes a path base: op U)
 *     X[i][j] = max(H[i][j-1] + o + e, X[i][j-1] + e)                                (consumes a read base: op L)
 *     H[i][j] = max(H[i-1][j-1] + sc(b_i, s_j), Y[i][j], X[i][j])
 *   CHOICE.  -m 6: the score of path k is H_k[m_k][n]; the highest score wins, ties go to the lowest path index; end_row is
 *     the path's last row.  -m 7: maximise H_k[i][n] over paths k and i >= 1; ties go to the smallest graph row, then to
 *     the lowest path index (the iteration order of best_ending_node, pathwise_alignment_semiglobal.rs:244-276); end_row
 *     is that row.
 *   TRACEBACK from state H at the chosen cell.  In H: D if H == H[i-1][j-1] + sc, else U (to state Y) if H == Y, else L (to
 *     state X): the project's D > U > L order.  In Y at (i, j): emit U; the run was opened at (i-1, j) (back to H) iff
 *     H[i-1][j] + o + e >= Y[i-1][j] + e, otherwise stay in Y (the reference's `u_dpm >= u_y` prefers opening likewise).  X
 *     is symmetric.  On the borders the walk follows the only finite state.  -m 6 ends at (0, 0); -m 7 ends when j == 0.
 *   RECORD.  Ops, best path, end row and score fill the record of -m 4, and the line is that mode's:
 *     "<cigar>, best path: k, score: S\t<path bases>".
 *   REFUSALS.  A read with a character outside ACGTN: RG_READ_BAD_BASE.  gap_open > 0 or gap_ext > 0, any amb_mode bit, a
 *     read longer than 2047 bases: RG_ERR_ARG.  (rows of the longest path + longest read) * max(|sc|, |o + e|) >= 2^28:
 *     RG_ERR_CAPACITY.  All of them are answered by rg_batch_create before a device is needed.
 * rg_batch_cell_updates counts rows_k * n per path and read; rg_batch_cell_updates_performed adds the direction pass of the
 * chosen path.
 */
#define RG_MODE_PATHWISE_GAP 6
#define RG_MODE_PATHWISE_GAP_SEMI 7
/*
 * RG_MODE_PATHWISE_GAP_LOCAL (12): LOCAL pathwise alignment with affine gaps (Smith-Waterman-Gotoh against every path): the
 * third member of the family above, for reads that are only partly on the graph (overhangs, adapters, chimeras).  Like modes 6
 * and 7 it is A DEFINITION OF THIS PROJECT'S OWN.  Inputs and score lookups are those of mode 6.
 *   RECURRENCE, independently for every path:
 *     H[0][j] = 0,  H[i][0] = 0;  X and Y are NEG on both borders
 *     Y[i][j] = max(H[i-1][j] + o + e, Y[i-1][j] + e)
 *     X[i][j] = max(H[i][j-1] + o + e, X[i][j-1] + e)
 *     H[i][j] = max(0, H[i-1][j-1] + sc(b_i, s_j), Y[i][j], X[i][j])
 *   CHOICE.  Maximise H_k[i][j] over paths k, i >= 1, 1 <= j <= n; ties go to the smallest graph row, then to the lowest path
 *     index (the order of mode 7), then to the smallest column.  end_row is that row, end_col = j.
 *   UNALIGNED.  If the maximum is 0 the read has no local alignment: status RG_READ_UNALIGNED, score 0, a record without ops.
 *     rg_result_gaf, rg_result_fields, rg_batch_format_all and the stream's text treat such a read as they treat a
 *     RG_READ_BAD_BASE read of a pathwise mode: it has no line.
 *   TRACEBACK from state H at (end_row, end_col).  In H: stop if H[i][j] == 0 (checked first); otherwise D if
 *     H == H[i-1][j-1] + sc, else U (to state Y) if H == Y, else L (to state X).  The Y and X states and their "prefer to have
 *     been opened" rule are those of mode 6.  The walk always ends on a cell with H == 0 (every border cell is one); stop_col
 *     is the column where it ends.
 *   RECORD and LINE.  The record and the comments of -m 4, "<cigar>, best path: k, score: S\t<path bases>", except that query
 *     start is stop_col, query end is end_col - 1 (inclusive, as modes 4-7 print 0 and n - 1), and CIGAR and path bases cover
 *     the aligned part only: clipped read bases appear nowhere else.  Path string, length, start and end are derived from (best
 *     path, end row, ops) as for mode 7.
 *   REFUSALS.  Those of modes 6 and 7, answered by rg_batch_create before a device is needed.
 * rg_batch_cell_updates counts rows_k * n per path and read; rg_batch_cell_updates_performed adds the direction pass, which
 * covers the rows of the chosen path up to the end row.
 */
#define RG_MODE_PATHWISE_GAP_LOCAL 12
/*
 * RG_MODE_PATHWISE_GAP_LONG (16), RG_MODE_PATHWISE_GAP_SEMI_LONG (17), RG_MODE_PATHWISE_GAP_LOCAL_LONG (22): the long-read
 * flavours of modes 6, 7 and 12, numbered `mode + 10` as the scalar flavours of modes 0 and 1 are.  THERE IS NO NEW RULE: mode
 * m + 10 is the definition of mode m above with one word changed — reads of 1 to 16383 bases.  Recurrence, choice, tie order,
 * traceback, record, line, RG_READ_UNALIGNED (mode 22) and both cell counters are those of mode m, and for every read of at
 * most 2047 bases mode m + 10 returns the bytes, the status and the score of mode m.
 *   REFUSALS.  gap_open > 0 or gap_ext > 0, any amb_mode bit, a read longer than 16383 bases: RG_ERR_ARG.  (rows of the longest
 *     path + longest read) * max(|sc|, |o + e|) >= 2^28: RG_ERR_CAPACITY.  All answered by rg_batch_create before a device is
 *     needed.
 *   COST.  A batch whose longest read has at most 2047 bases runs exactly as in mode m.  Otherwise every read of the batch is
 *     aligned in column stripes of 2048 (a read of n bases runs ceil((n + 1) / 2048) of them), and the direction words of the
 *     chosen path take stripes * (rows of the longest path + 1) * 1 KiB per read of the batch: about 140 MB for one 16383-base
 *     read on 17000 rows.  Modes 6, 7 and 12 themselves keep their limit of 2047 bases.
 */
#define RG_MODE_PATHWISE_GAP_LONG 16
#define RG_MODE_PATHWISE_GAP_SEMI_LONG 17
#define RG_MODE_PATHWISE_GAP_LOCAL_LONG 22
/*
 * RG_MODE_PATHWISE_GAP_STRANDS (26), RG_MODE_PATHWISE_GAP_SEMI_STRANDS (27), RG_MODE_PATHWISE_GAP_LOCAL_STRANDS (32): modes 6, 7
 * and 12 on BOTH STRANDS, numbered `mode + 20`.  Write "pipeline m" for the long flavour 16, 17 or 22 of the base mode: the new
 * modes take reads of 1 to 16383 bases, and every pass of theirs is one run of pipeline m (a pass without a read over 2047 bases
 * runs the base mode's kernels).  THERE IS NO NEW RECURRENCE, CHOICE, TRACEBACK OR LINE; what is new is which strand is reported.
 * RG_AMB_BOTH_STRANDS and RG_AMB_STRAND_VOTE are defined below.
 *   MODES 26 AND 27, amb_mode 0 or 4 (bit 2 is implied and accepted as redundant): THE EXACT RULE.  Rules 1 to 5 of
 *     RG_AMB_BOTH_STRANDS word for word, "the pipeline" being pipeline 16 or 17 and the score the integer the record prints: a
 *     read qualifies for the reverse pass iff its status has neither RG_READ_BAD_BASE nor RG_READ_WOULD_PANIC and its forward
 *     score is < 0; the reverse record wins only when its score is STRICTLY greater; a winning reverse read is reported exactly
 *     as its reverse complement would be had it been submitted by itself in mode 16 or 17, except for strand column '-'.
 *     CONSEQUENCE: a batch in which no forward score is negative returns the bytes, statuses and scores of mode 16 or 17.
 *   MODES 26 AND 27, amb_mode 12: THE VOTE RULE.  Rules 1 to 7 of RG_AMB_STRAND_VOTE verbatim, pass A and pass B being pipeline
 *     16 or 17.
 *   MODE 32, amb_mode 0 or 4.  A local score is never negative, so a `< 0` gate could never fire.  Here EVERY read whose forward
 *     status has neither RG_READ_BAD_BASE nor RG_READ_WOULD_PANIC is also aligned as its reverse complement, and the reverse
 *     record wins only when its score is STRICTLY greater.  An RG_READ_UNALIGNED record has score 0: forward unaligned and
 *     reverse aligned — the reverse record, status 0; both unaligned — RG_READ_UNALIGNED, strand '+', no line; ties (a
 *     reverse-palindromic read included) — forward.  Query start and query end of a chosen reverse record are in the reverse
 *     complement's coordinates (rule 5).  amb_mode 12 is RG_ERR_ARG in mode 32: no score of a local pass says "hopeless", so a
 *     vote would have no pass-B rule.
 *   REFUSALS.  amb_mode bits 0 and 1, bit 3 alone, any higher bit, and everything modes 16, 17 and 22 refuse (positive gap
 *     costs, a read over 16383 bases: RG_ERR_ARG; the 2^28 budget: RG_ERR_CAPACITY).  All answered by rg_batch_create before a
 *     device is needed.
 * Both cell counters include pass B.  k_strand_gate (mode 32: k_gap_strands_gate), k_revcomp and k_strand_merge appear in the
 * kernel statistics under their own names, with amb_mode 12 also k_strand_vote and k_strand_orient.
 */
#define RG_MODE_PATHWISE_GAP_STRANDS 26
#define RG_MODE_PATHWISE_GAP_SEMI_STRANDS 27
#define RG_MODE_PATHWISE_GAP_LOCAL_STRANDS 32
/*
 * RG_MODE_PATHWISE_GAP_XLONG (56), RG_MODE_PATHWISE_GAP_SEMI_XLONG (57), RG_MODE_PATHWISE_GAP_LOCAL_XLONG (62): modes 6, 7 and 12 for
 * reads of 1 to 131071 bases (64 column stripes of 2048), numbered `mode + 50`.  THERE IS NO NEW RULE: mode m + 50 is the definition
 * of mode m with the read length changed.  Recurrence, choice, tie order, traceback, record, line, RG_READ_UNALIGNED (mode 62) and
 * rg_batch_cell_updates are those of mode m; for every read of at most 16383 bases mode m + 50 returns the bytes, the status and the
 * score of mode m + 10, hence those of mode m for reads of at most 2047 bases.
 *   REFUSALS.  gap_open > 0 or gap_ext > 0, any amb_mode bit (both strands at this length is not offered), a read longer than
 *     131071 bases: RG_ERR_ARG.  (rows of the longest path + longest read) * max(|sc|, |o + e|) >= 2^28: RG_ERR_CAPACITY.  All
 *     answered by rg_batch_create before a device is needed.
 *   COST.  A batch whose longest read has at most 2047 bases runs exactly as in mode m.  Otherwise the traceback keeps the direction
 *     words of ONE stripe per read, (rows of the longest path + 1) * 1 KiB, and per row of the chosen path two integers for each
 *     stripe but the last: the walk only ever moves left, so each stripe's words are rebuilt from its checkpoint when the walk
 *     enters it, once.  rg_batch_cell_updates_performed counts the score pass, the checkpoint pass (rows * n per read) and the
 *     rebuilt cells (rows rebuilt * the stripe's columns that belong to the read).  Modes 16, 17, 22, 26, 27 and 32 keep their
 *     limit of 16383 bases and their kernels.
 */
#define RG_MODE_PATHWISE_GAP_XLONG 56
#define RG_MODE_PATHWISE_GAP_SEMI_XLONG 57
#define RG_MODE_PATHWISE_GAP_LOCAL_XLONG 62
/*
 * RG_MODE_PATHWISE_GAP_XSTRANDS (76), RG_MODE_PATHWISE_GAP_SEMI_XSTRANDS (77), RG_MODE_PATHWISE_GAP_LOCAL_XSTRANDS (82): modes 6, 7
 * and 12 on BOTH STRANDS for reads of 1 to 131071 bases, numbered `mode + 70`.  Write "pipeline m" for mode 56, 57 or 62 of the base
 * mode.  THERE IS NO NEW RECURRENCE, CHOICE, TIE ORDER, TRACEBACK, RECORD OR LINE; what is new is which strand is reported, and that
 * rule is mode m + 20's, restated on the PICKED scores.  A read's PICK on a strand is (status, score, path, end row) as the score
 * pass and the pick of pipeline m leave it: the score that decides between the strands is that integer, which no traceback changes.
 *   MODES 76 AND 77, amb_mode 0 or 4 (bit 2 is implied and accepted as redundant): every read is picked forward; a read whose
 *     forward pick has neither RG_READ_BAD_BASE nor RG_READ_WOULD_PANIC and a score < 0 is also picked as its reverse complement;
 *     the reverse strand wins only when its pick has a record and a STRICTLY greater score.
 *   MODES 76 AND 77, amb_mode 12: rules 1 to 7 of RG_AMB_STRAND_VOTE with "pass" read as "pick": the first strand by the 12-mer
 *     vote, a read goes to the second pick iff its first score is < 0, reverse wins only if strictly greater, whichever went first.
 *   MODE 82, amb_mode 0 or 4: every read without RG_READ_BAD_BASE is picked on both strands, and reverse wins only if strictly
 *     greater.  An RG_READ_UNALIGNED pick scores 0: forward unaligned and reverse aligned — reverse, status 0; both unaligned —
 *     RG_READ_UNALIGNED, strand '+', no line; ties and reverse-palindromic reads — forward.  amb_mode 12 is RG_ERR_ARG, for mode
 *     32's reason: no score of a local pass says "hopeless", so a vote would have no rule for a second pass.
 *   REPORTING.  The winning strand ALONE is traced.  The read is reported exactly as that strand's sequence would be had it been
 *     submitted by itself in mode m + 50, except for strand column '-' of a reverse winner; query coordinates of mode 82 are in the
 *     reverse complement's coordinates.  Every accessor, rg_batch_format_all and a stream's text describe the chosen record.
 *   WHERE THE WORDING DIFFERS FROM MODES 26 / 27 / 32.  There a read qualifies by the status of its finished RECORD, here by that of
 *     its PICK: an RG_READ_WOULD_PANIC that only the walk could raise can no longer keep a read from its reverse pick.  For a batch
 *     the plan admits the walk cannot raise one: it starts on the pick's end row, which is a row of the picked path (its index + 1
 *     is at most the rows of the longest path, the geometry every buffer is sized for); every emitted op moves one row up or one
 *     column left from at most (rows of the path, n), so a walk has at most rows + n ops, below the op area of a read, min(rows of the
 *     graph + longest read + 8, 2 (rows of the longest path + longest read) + 16); its iteration cap 3 (rows + n) + 3 covers every
 *     valid walk; and the local kind's end column is the one the same integer row step found in the score pass.  CONSEQUENCE: for every
 *     read of at most 16383 bases, mode m + 70 returns the bytes, statuses and scores of mode m + 20 with the same amb_mode.
 *   REFUSALS.  amb_mode bits 0 and 1, bit 3 alone, any higher bit, positive gap costs, a read over 131071 bases: RG_ERR_ARG.  The
 *     2^28 budget of modes 56, 57, 62: RG_ERR_CAPACITY.  All answered by rg_batch_create before a device is needed.  Modes 56, 57 and
 *     62 keep refusing every amb_mode bit; modes 26, 27 and 32 keep their limit of 16383 bases.
 *   COUNTERS.  rg_batch_cell_updates = rows_k * n summed over the paths, for every (read, strand) that was picked.
 *     rg_batch_cell_updates_performed adds the traceback cells of the traced strand only: mode m + 50's formula for that strand.
 * k_gap_pick_out, k_gap_seed_pick, k_gap_xstrands_duel and k_gap_xstrands_mark (gap_xstrands/) appear in the kernel statistics
 * under their own names beside the gate, k_revcomp and k_strand_orient; there is no k_strand_merge and no second op area.
 */
#define RG_MODE_PATHWISE_GAP_XSTRANDS 76
#define RG_MODE_PATHWISE_GAP_SEMI_XSTRANDS 77
#define RG_MODE_PATHWISE_GAP_LOCAL_XSTRANDS 82
/*
 * RG_MODE_PATHWISE_EDIT (44), RG_MODE_PATHWISE_EDIT_SEMI (45): modes 16 and 17 RESTRICTED TO UNIT COSTS (match 0; mismatch, inserted
 * and deleted base 1: edit distance against every path), computed with Myers' bit-vector recurrence: one cell per bit instead of one
 * per register, a read of up to 16383 bases whole in one wave.  THERE IS NO NEW RULE: for every batch they admit, mode 44 returns the
 * bytes, statuses, scores and both cell counters that mode 16 returns for the same rg_params, mode 45 those of mode 17 (recurrence,
 * choice, tie order, traceback, record, line and RG_READ_BAD_BASE reads included).  The modes are values of rg_params.mode only: no
 * entry point, no struct field, and no row of the affine-gap family table.
 *   ADMISSION.  gap_open == 0 and gap_ext == -1, and every entry scores[a * 6 + b] with a, b < 5 (the ACGTN x ACGTN block) is 0 or
 *     -1: `-M 0 -X 1 -O 0 -E 1`, or any 0 / -1 matrix (an N that matches N, for one).  The '-' entries are not looked at.
 *   REFUSALS.  Other gap costs or block entries (the message names `-M 0 -X 1 -O 0 -E 1`), any amb_mode bit (the reads are aligned as
 *     given), a read longer than 16383 bases, and whatever else mode 16 refuses: RG_ERR_ARG (the 2^28 budget of mode 16:
 *     RG_ERR_CAPACITY).  All answered by rg_batch_create before a device is needed.
 *   WHY THE BYTES AGREE.  With costs in {0, 1} every difference between neighbouring cells of the distance matrix is -1, 0 or +1, so
 *     a row is two bit vectors and a row step a handful of word operations with one wide addition; with o = 0 every gap state of the
 *     rule of mode 6 equals H, and its traceback reads: D if H == H[i-1][j-1] + sc, else U if H == H[i-1][j] - 1, else L.  The
 *     direction pass keeps two bits per cell from which the walk decides exactly that ("the diagonal is equal", "the vertical
 *     difference is +1"); whether the two bases match is recomputed from the bases.
 *   COST.  The direction bits of the chosen path take (rows of the longest path + 1) * W * 512 bytes per read of the batch, W = 1, 2,
 *     4 or 8 the smallest with longest read <= 2048 W: about 70 MB for one 16383-base read on 17000 rows, half of mode 16's.
 * k_edit_score, k_edit_dirs and k_edit_trace (edit/rg_path_edit.hip) appear in the kernel statistics under their own names beside
 * k_gap_pick, which is the kernel of modes 6 and 7.
 */
#define RG_MODE_PATHWISE_EDIT 44
#define RG_MODE_PATHWISE_EDIT_SEMI 45
/*
 * RG_MODE_PATHWISE_EDIT_XLONG (94), RG_MODE_PATHWISE_EDIT_SEMI_XLONG (95): modes 44 and 45 for reads of 1 to 131071 bases, numbered
 * `mode + 50` as the xlong family is.  THERE IS NO NEW RULE: mode 94 is mode 56, and mode 95 is mode 57, RESTRICTED TO UNIT COSTS.
 * For every batch they admit they return the texts, statuses, scores and rg_batch_cell_updates of mode 56 / 57 under the same
 * rg_params; for a batch whose longest read has at most 16383 bases they return everything of mode 44 / 45, both counters included,
 * from that mode's plan and kernels.
 *   ADMISSION AND REFUSALS.  Those of modes 44 / 45 (unit costs — the message names `-M 0 -X 1 -O 0 -E 1` —, no amb_mode bit, mode 16's
 *     2^28 budget as RG_ERR_CAPACITY) with the read limit at 131071 bases.  All answered by rg_batch_create before a device is needed.
 *     Modes 44 and 45 keep their limit of 16383 bases.
 *   COST.  A batch with a longer read runs S = ceil(longest read / 16384) column stripes of 16384, 2 <= S <= 8 (16384 bases: 2), each in the register
 *     layout of W = 8, one wave per (read, path) walking them in turn.  What a stripe hands to its right neighbour is the difference
 *     of its last column between two rows, -1, 0 or +1: two bits per row, kept for every stripe but the last of EVERY path, so the
 *     traceback needs no checkpoint pass.  It keeps D0 and Ph of ONE stripe per read, (rows of the longest path + 1) * 4 KiB, rebuilt
 *     from the picked path's boundary bits when the walk enters the stripe, once.  rg_batch_cell_updates_performed counts the score
 *     pass and the rebuilt cells (rows rebuilt * the stripe's columns that belong to the read; cell (i, j) is of stripe (j - 1) / 16384).
 * k_edit_score_xlong, k_edit_redo_xlong and k_edit_walk_xlong (edit_xlong/rg_path_edit_xlong.hip) appear in the kernel statistics
 * under their own names beside k_gap_pick.
 */
#define RG_MODE_PATHWISE_EDIT_XLONG 94
#define RG_MODE_PATHWISE_EDIT_SEMI_XLONG 95
/*
 * RG_MODE_PATHWISE_EDIT_STRANDS (64), RG_MODE_PATHWISE_EDIT_SEMI_STRANDS (65): modes 44 and 45 on BOTH STRANDS, for reads of 1 to
 * 16383 bases.  THERE IS NO NEW RULE: for every batch they admit, every read's text, status, score, strand and query coordinates are
 * those of mode 26 (mode 64) or mode 27 (mode 65) under the same rg_params with amb_mode 0: modes 6 / 7 on both strands at unit costs.
 *   DECISION.  A read without RG_READ_BAD_BASE is picked on BOTH strands in one pass (the pick of modes 6 / 7 and its tie rules, per
 *     strand); the reverse strand wins only when its pick has a record and a STRICTLY greater score.  Ties and reverse-palindromic
 *     reads stay '+'.  WHY THIS IS THE `< 0` GATE OF MODES 26 / 27: at unit costs every score is <= 0.  A read with forward score < 0
 *     passes the gate there and is picked on both strands here; a read with forward score 0 does not pass the gate there, and here
 *     no reverse score can be strictly greater than 0, so forward stays.  Both give the same strand for every read.
 *   REPORTING.  The winning strand ALONE is traced.  The read is reported exactly as that strand's sequence would be had it been
 *     submitted by itself in mode 44 / 45, with strand column '-' for a reverse winner.  A read with a bad base: its status, no
 *     line, strand '+'.
 *   ADMISSION.  Unit costs exactly as modes 44 / 45; reads of at most 16383 bases; mode 16's 2^28 budget (RG_ERR_CAPACITY).  amb_mode 0
 *     or 4: bit 2 is implied and accepted as redundant.
 *   REFUSALS (RG_ERR_ARG).  amb_mode 12: a vote saves nothing when both strands are scored in one pass, and would change the rule.
 *     amb_mode bits 0 and 1, bit 3 alone, any higher bit.  Any other scoring: the message names `-M 0 -X 1 -O 0 -E 1`, and -m 26 /
 *     -m 27 for every other scoring.  All answered by rg_batch_create before a device is needed.
 *   COUNTERS.  rg_batch_cell_updates = 2 * n * (rows_k summed over the paths), summed over the reads without a bad base: BOTH strands
 *     of every read are always scored — the one place these modes differ from modes 26 / 27, which count the reverse strand of the
 *     gated reads only.  rg_batch_cell_updates_performed adds mode 44 / 45's direction-pass term for the traced strand only.
 *   NOT OFFERED.  Reads over 16383 bases (the striped kernels of modes 94 / 95 keep the boundary bits of the score pass for the walk:
 *     two strands would double up to 206 MB per read), the 12-mer vote, a local rule.  Modes 44, 45, 94 and 95 keep refusing every
 *     amb_mode bit.
 * k_edit_score_pair (one wave scores both strands of a (read, path): the read in lanes 0 to 31, its reverse complement in lanes 32 to
 * 63) and k_edit_strands_duel (edit_strands/rg_edit_strands.hip) appear in the kernel statistics under their own names beside
 * k_gap_pick (twice per chunk), k_strand_orient, k_edit_dirs, k_edit_trace and k_gap_xstrands_mark.
 */
#define RG_MODE_PATHWISE_EDIT_STRANDS 64
#define RG_MODE_PATHWISE_EDIT_SEMI_STRANDS 65

/*
 * Scoring and banding parameters.  Replaces the HashMap<(char,char),i32|f32> score matrix arguments
 * (score_matrix.rs:35-51; api.rs:131,153) and the scalar arguments of the exec functions.
 * scores[a*6+b] is the entry for the key (ALPHA[a], ALPHA[b]) with ALPHA = "ACGTN-"; RG_SCORE_MISSING
 * marks a key the map does not hold.
 */
#define RG_SCORE_MISSING (-536870912)
typedef struct rg_params {
    int32_t mode;          /* RG_MODE_*                                                       */
    int32_t scores[36];
    int32_t gap_open;      /* o  (<= 0), gap_global_abpoa.rs:16                                */
    int32_t gap_ext;       /* e  (<= 0), gap_global_abpoa.rs:17                                */
    float band_b;          /* -b, main.rs:57: bta = (b + f * (n+1)) as usize                   */
    float band_f;          /* -f                                                              */
    int64_t bta_override;  /* >= 0: use this bases_to_add for every read (api.rs:22 callers)   */
    int32_t base_rec_cost; /* -R, pathwise_alignment_recombination.rs:29                       */
    float multi_rec_cost;  /* -r                                                              */
    float rec_band_width;  /* -B                                                              */
    int32_t amb_mode;      /* POA modes, `-s true` retry (main.rs:82-106): bit 0 = node ids of the reversed handle
                              order (utils.rs:144-165 with amb_mode), bit 1 = strand '-' (gaf_output.rs:225).
                              Pathwise modes: bit 2 = RG_AMB_BOTH_STRANDS, bit 3 = RG_AMB_STRAND_VOTE (below; bit 3 only
                              together with bit 2); bits 0 and 1 are refused there, bits 2 and 3 in the POA modes    */
} rg_params;

/*
 * RG_AMB_BOTH_STRANDS (bit 2 of rg_params.amb_mode; modes 4, 5, 8, 9 only): both strands inside one batch.  AN
 * EXTENSION THE REFERENCE DOES NOT HAVE: its `-s true` covers modes 0-3 (main.rs:82-106, 132-165, 188-212, 229-253) and
 * is ignored by the pathwise modes (main.rs:254-313), as rg_stream_opts.amb_strand = 1 still is here.  Opt-in:
 *   1. every read is aligned as given (the forward pass: the pipeline without the bit);
 *   2. a read QUALIFIES for the reverse pass when its status has neither RG_READ_BAD_BASE nor RG_READ_WOULD_PANIC and its
 *      forward score is < 0 (the reference's rule for the global POA modes, main.rs:82).  The score is the number the
 *      record prints after "score: ": the integer in -m 4 / 5 and for a -m 8 / 9 record without a recombination, the f32
 *      of a record with one; compared as f32 (every integer involved is below 2^24);
 *   3. the reverse complement of each qualifying read (sequences.rs:65-82: reversed, A<->T, C<->G, N stays) is aligned
 *      against the same forward graph with the same parameters, on the device, in the handle's own work buffers;
 *   4. the reverse record replaces the forward one only when its score is STRICTLY greater; ties keep the forward one;
 *   5. a read whose reverse record won is reported exactly as its reverse complement would be had it been submitted by
 *      itself (path, coordinates, CIGAR, score, query length), except that the strand column is '-'.  rg_result_score,
 *      rg_result_status, rg_result_fields().strand, rg_result_gaf, rg_batch_format_all and a stream's text / score /
 *      status describe the record that was chosen.  Node ids are NOT relabelled (a PathGraph has no reversed handle
 *      order: bit 0 stays POA-only).
 * rg_batch_cell_updates and rg_batch_cell_updates_performed include the second pass (the workload grew); the kernels of
 * the second pass add to the time and launches of their names, and k_strand_gate, k_revcomp, k_strand_merge appear
 * under their own.  For the POA modes the way to both strands is rg_stream_opts.amb_strand (`-s true`).
 */
#define RG_AMB_BOTH_STRANDS 4

/*
 * RG_AMB_STRAND_VOTE (bit 3 of rg_params.amb_mode; valid only together with bit 2, so amb_mode = 12, and only in modes
 * 4, 5, 8, 9): RG_AMB_BOTH_STRANDS with the FIRST strand picked per read by a 12-mer vote, so that a read of the other
 * strand is not first aligned as a hopeless forward read.  The vote is a pure function of (graph, read); the rule, a
 * second one beside the exact rule above:
 *   1. VOTES.  K = 12; for a read of n bases npos = n - 11.  npos < 1: both votes are 0.  Otherwise step =
 *      ceil(npos / 256) and the samples are the windows that start at t * step for t * step < npos (at most 256).  V_f =
 *      the number of sampled windows of the read that consist of A/C/G/T only and occur as a 12-mer of some path of the
 *      graph (exact set membership).  V_r = the same count for the reverse complement of the read, sampled in the
 *      reverse complement's own coordinates.  A read with RG_READ_BAD_BASE votes 0 / 0.
 *   2. FIRST STRAND.  '-' iff V_r > V_f; ties go to '+'.
 *   3. PASS A aligns every read on its first strand (one pass of the pipeline).
 *   4. PASS B.  A read goes to pass B iff its pass-A status has neither RG_READ_BAD_BASE nor RG_READ_WOULD_PANIC and its
 *      pass-A score (the printed score of rule 2 above) is < 0.  Pass B aligns the other strand.
 *   5. CHOICE.  One strand aligned: that record.  Both aligned: the reverse record only if its score is STRICTLY greater;
 *      ties keep forward, whichever strand went first.  A pass that yields no record never wins.
 *   6. REPORTING as rule 5 above: strand column '-' for a chosen reverse record, and every accessor and a stream's text,
 *      score and status describe the chosen record.
 *   7. WHERE IT DIFFERS FROM THE EXACT RULE: only for a read that goes reverse first and whose reverse score is >= 0.  Its
 *      forward strand is then never looked at, while RG_AMB_BOTH_STRANDS alone would have kept the forward record
 *      whenever forward >= 0 or forward >= reverse.
 * k_strand_vote and k_strand_orient appear in the kernel statistics under their own names; both cell counters include
 * pass B.  Bit 3 alone, and bit 3 in a POA mode, are RG_ERR_ARG.
 */
#define RG_AMB_STRAND_VOTE 8

/* Fill *p with the CLI defaults (args_parser.rs:3-147: M=2 X=4 O=4 E=2 R=4 r=0.1 B=1 b=1 f=0.01). */
void rg_params_default(rg_params* p, int32_t mode);
/* score_matrix::create_score_matrix_match_mis (score_matrix.rs:35-51); f32_variant=1 gives
 * create_score_matrix_match_mis_f32 (:52-66, gap = mismatch). */
void rg_scores_match_mis(int32_t match, int32_t mismatch, int32_t f32_variant, int32_t* scores36);

typedef struct rg_graph rg_graph;
typedef struct rg_batch rg_batch;

/*
 * Graph ingestion.  Replaces graph::read_graph / create_graph_struct (graph.rs:11-102),
 * pathwise_graph::read_graph_w_path / create_path_graph / create_reverse_path_graph /
 * nodes_displacement_matrix (pathwise_graph.rs:127-305), utils::set_r_values (utils.rs:103-126) and
 * utils::create_handle_pos_in_lnz (utils.rs:144-165).  The flattened graph is uploaded to HBM once.
 */
int32_t rg_graph_from_gfa(const char* gfa_text, int64_t len, rg_graph** out);
/* Same, from an already flattened LnzGraph (graph.rs:23-27): pred rows of row i are
 * pred_rows[pred_off[i] .. pred_off[i+1]) in pred_hash order, nwp[i] = pred_off[i+1] > pred_off[i],
 * node_id[i] = segment id of row i (0 for row 0 and the final 'F' row). */
int32_t rg_graph_create_lnz(const char* lnz, int64_t L, const int64_t* pred_off, const int64_t* pred_rows,
                            const uint64_t* node_id, rg_graph** out);
/* Same, from an already flattened PathGraph (pathwise_graph.rs:10-18).  Path sets are W = (P + 63) / 64 words each: bit
 * (k & 63) of word (k >> 6) of row_mask[i * W ..] = paths_nodes[i][k]; edges of row i are (edge_pred[e],
 * edge_mask[e * W ..]) for e in [edge_off[i], edge_off[i+1]) (PredHash, pathwise_graph.rs:75-125; listed for
 * segment-start rows and the 'F' row).  P <= 256. */
int32_t rg_graph_create_path(const char* lnz, int64_t L, int32_t P, const uint64_t* row_mask,
                             const int64_t* edge_off, const int64_t* edge_pred, const uint64_t* edge_mask,
                             const uint64_t* node_id, rg_graph** out);
void rg_graph_destroy(rg_graph* g);
/* A GFA whose P lines cannot be turned into a PathGraph (more than 256 paths, '-' path steps, a step on an unknown
 * segment, steps against the id order, a segment on no path: pathwise_graph.rs:182) still yields the LnzGraph view, which
 * is all modes 0-3 need (main.rs:29); the reason is returned here ("" when the PathGraph view exists or the GFA has no
 * P lines) and by rg_batch_create (RG_ERR_GRAPH) when a pathwise mode is requested on such a graph.
 * Limits of the pathwise kernels: at most 256 paths; reads of at most 16383 bases (reads longer than 2047 bases run
 * as column stripes of 2048 in one workgroup and need a uniform read-gap cost: every matrix the reference's CLI builds). */
const char* rg_graph_path_error(const rg_graph* g);
int64_t rg_graph_rows(const rg_graph* g);   /* lnz.len() of the LnzGraph (or PathGraph if only that exists) */
int32_t rg_graph_paths(const rg_graph* g);  /* paths_number, 0 without P lines */
/* text dumps of the flattened arrays (same `which` codes as the test oracle) for construction tests */
int64_t rg_graph_dump(const rg_graph* g, int32_t which, char* buf, int64_t cap);

/*
 * Batch alignment.  One call replaces the reference's per-read loop (main.rs:56-105, 174-213,
 * 257-261, 297-312): reads are bases without the leading '$' (sequences.rs:5-45 is applied inside:
 * upper-casing and '-' -> 'N'); read i is reads[read_off[i] .. read_off[i+1]).
 *
 *   rg_batch_create   uploads the reads and sizes every work buffer in HBM
 *   rg_batch_run      runs the DP + traceback kernels on the device (inputs resident; this is the
 *                     region bench.py times); may be called repeatedly
 *   rg_batch_fetch    copies the alignment records back (one D2H of packed records)
 *   rg_result_*       per-read accessors; rg_result_gaf formats exactly what the reference prints on
 *                     stdout for that read (warning lines + GAFStruct::to_string, gaf_output.rs:70-94)
 */
int32_t rg_batch_create(const rg_graph* g, const rg_params* p, const char* reads, const int64_t* read_off,
                        int64_t nreads, rg_batch** out);
/* Replaces the reads of an existing batch handle (same graph, same parameters) and uploads them: a streaming caller
 * keeps one or two handles and their HBM work buffers for the whole read set instead of re-creating them per chunk of
 * the reference's read loop (main.rs:56,174,257,297).  Results of the previous reads are discarded. */
int32_t rg_batch_set_reads(rg_batch* b, const char* reads, const int64_t* read_off, int64_t nreads);
int32_t rg_batch_run(rg_batch* b);
int32_t rg_batch_fetch(rg_batch* b);
void rg_batch_destroy(rg_batch* b);

int64_t rg_batch_size(const rg_batch* b);
uint32_t rg_result_status(const rg_batch* b, int64_t i);
int32_t rg_result_score(const rg_batch* b, int64_t i);   /* exec(..).0 of the reference (POA modes); best score otherwise */
/* seq_index is seq_name.1 of the reference (0 = score only: empty text). Returns bytes needed (excl. NUL). */
int64_t rg_result_gaf(const rg_batch* b, int64_t i, const char* name, int64_t seq_index, char* buf, int64_t cap);

/* Structured form of the same record: the fields of the reference's GAFStruct (gaf_output.rs:6-20) so that a caller
 * (the Rust shim under shim/) builds its GAFStruct without parsing text.  query_name is the caller's.  Strings are not
 * owned by the library: the node ids of `path` go to path_ids[0 .. n_path_ids) and `comments` (NUL-terminated) to
 * comments[] when the capacities suffice; call once with null buffers to learn the sizes.  alignment_block_length and
 * mapping_quality are "*" unless `empty` is set (GAFStruct::new(), gaf_output.rs:22-38: both "", strand ' ', path [0]). */
typedef struct rg_gaf_fields {
    int32_t has_record;          /* 0: the reference returns no GAFStruct for this read (it panics: see rg_result_status) */
    int32_t empty;               /* 1: GAFStruct::new() ("band not enough for correct output", gaf_output.rs:861-864) */
    uint32_t warning;            /* RG_READ_BAND_WARNING / RG_READ_BAND_NOT_ENOUGH: the stdout line printed before the record */
    char strand;
    uint64_t query_length, query_start, query_end;
    uint64_t path_length, path_start, path_end;
    uint64_t residue_matches_number;
    int64_t n_path_ids;
    int64_t comments_len;        /* bytes, excluding the NUL */
} rg_gaf_fields;
int32_t rg_result_fields(const rg_batch* b, int64_t i, rg_gaf_fields* out, uint64_t* path_ids, int64_t path_cap, char* comments,
                         int64_t comments_cap);

/* Formats every read of the batch (as rg_result_gaf would, name i = names[i] or "read<i>" when names is
 * NULL, seq_index = seq_index_base + i) into one buffer using `nthreads` host threads; returns bytes needed. */
int64_t rg_batch_format_all(const rg_batch* b, const char* const* names, int64_t seq_index_base, char* buf,
                            int64_t cap, int32_t nthreads);

/* Measurement hooks for bench.py: DP cell-updates of the last run (SURVEY §8d unit of work) and
 * per-kernel device time measured with HIP events on the stream the kernels were launched on. */
uint64_t rg_batch_cell_updates(const rg_batch* b);
/* The cell updates the kernels actually performed for that workload: the same number except where k_sweep16 runs a
 * segment's rows as a gather run (per row the alpha and a column map instead of one update per member path) and where
 * its -m 8 sweeps retire paths (a path that provably cannot matter any more, and leads no path that can,
 * is not updated further; the results are the same bytes).  The updates of a second pass after a failed speculation count
 * here (they are work the device performed) and not in rg_batch_cell_updates (the workload did not grow). */
uint64_t rg_batch_cell_updates_performed(const rg_batch* b);
int32_t rg_batch_kernel_count(const rg_batch* b);
const char* rg_batch_kernel_name(const rg_batch* b, int32_t k);
double rg_batch_kernel_ms(const rg_batch* b, int32_t k);       /* summed over launches of the last run */
int64_t rg_batch_kernel_launches(const rg_batch* b, int32_t k);

/* one-shot convenience: create + run + fetch */
int32_t rg_align_batch(const rg_graph* g, const rg_params* p, const char* reads, const int64_t* read_off,
                       int64_t nreads, rg_batch** out);

/*
 * The same read loop over several GPUs behind ONE call (the reference loop main.rs:56,174,257,297 has no order
 * dependence between reads): the reads go through the streaming engine below (tiles pulled from one queue by the
 * batch handles of every device in device_ids, NULL: every visible device; the graph tables are uploaded once per
 * device; nothing is exchanged between devices) and the call returns when the last tile is done.  Shard k is one tile:
 * it holds reads [begin_k, begin_{k+1}) as a results-only rg_batch, owned by the rg_multi, for the rg_result_* accessors
 * (rg_batch_run / rg_batch_set_reads refuse it); rg_multi_format_all concatenates the text of all shards in input
 * order (names[i], seq_index_base + i index the whole read set).  With names == NULL the default name of read i is
 * "read<j>", j = its index inside its shard (as rg_batch_format_all): pass names for global numbering.
 */
typedef struct rg_multi rg_multi;
int32_t rg_align_batch_multi(const rg_graph* g, const rg_params* p, const char* reads, const int64_t* read_off,
                             int64_t nreads, const int32_t* device_ids, int32_t ndev, rg_multi** out);
int32_t rg_multi_shards(const rg_multi* m);
rg_batch* rg_multi_batch(const rg_multi* m, int32_t k);
int64_t rg_multi_shard_begin(const rg_multi* m, int32_t k);      /* k == shards: nreads */
int64_t rg_multi_format_all(const rg_multi* m, const char* const* names, int64_t seq_index_base, char* buf, int64_t cap,
                            int32_t nthreads);
void rg_multi_destroy(rg_multi* m);

/*
 * FASTA ingestion.  Replaces sequences::get_sequences (sequences.rs:5-45) with the same rules: a line that starts with
 * '>' names a read (everything after the '>') and closes the read before it when that one has bases; every other
 * non-empty line is appended to the current read, upper-cased, '-' -> 'N'; lines end at '\n' with one '\r' before it
 * dropped (BufRead::lines); the reads are paired with the names BY INDEX, and a file whose counts differ is refused
 * (RG_ERR_ARG, "wrong fasta file format": the reference panics, :41-43).  The '$' the reference puts in front of
 * every read is added inside the library.  bases / offsets / names are the input form of rg_batch_create,
 * rg_stream_push and rg_align_batch_multi and stay valid until rg_reads_destroy.
 */
typedef struct rg_reads rg_reads;
int32_t rg_reads_from_fasta(const char* fasta_text, int64_t len, rg_reads** out);
int64_t rg_reads_count(const rg_reads* r);
const char* rg_reads_bases(const rg_reads* r);            /* concatenated bases of all reads */
const int64_t* rg_reads_offsets(const rg_reads* r);       /* count + 1 offsets into bases */
const char* const* rg_reads_names(const rg_reads* r);     /* count NUL-terminated names */
void rg_reads_destroy(rg_reads* r);
/* The check of sequences.rs:41-43 without keeping anything: the reference parses the whole file (and panics with "wrong
 * fasta file format" when the name and sequence counts differ) BEFORE it aligns the first read; a caller that streams
 * a file through rg_stream_feed_fasta runs this over the same blocks ahead of its first output.  state4: four words,
 * zero before the first piece.  Returns RG_ERR_ARG at the final piece of a text the reference refuses; *nreads_out:
 * reads so far. */
int32_t rg_fasta_check(const char* piece, int64_t len, int32_t final, int64_t* state4, int64_t* nreads_out);

/*
 * Streaming engine: the reference's read loop (main.rs:56,174,257,297-312) as a pipeline hidden behind the boundary.
 * Reads pushed into a stream are cut into tiles; per device `handles_per_device` batch handles (each with its own HIP
 * stream, HBM work buffers and host thread) pull tiles from ONE queue shared by all devices of the stream (a tile goes
 * to whichever handle is free first: load balance across devices without a static split), upload, align, fetch and
 * format them; the latency-bound small kernels of one tile run beside the sweeps of the others and the host work
 * (canonicalisation, upload, record fetch, GAF formatting on `format_threads` threads) overlaps the device work of
 * the other handles.  Results come back in input order, one tile per rg_stream_next call, as exactly the bytes the
 * reference prints on stdout for those reads.  Nothing is exchanged between devices.
 *
 *   rg_stream_create   starts the worker threads (the device buffers are allocated by the first tiles)
 *   rg_stream_push     copies the reads (and names) and queues their tiles; returns at once; any thread, any time
 *                      before rg_stream_finish.  names == NULL: read i of the stream is called "read<i>"
 *   rg_stream_finish   no more pushes: rg_stream_next returns RG_STREAM_END after the last tile
 *   rg_stream_next     blocks until the next tile (in input order) is done.  A tile whose device work failed returns
 *                      that error (rg_last_error has the text) and the stream moves on to the next tile
 *
 * seq_index of read i is seq_index_base + i (main.rs passes i + 1 in modes 0-3, where 0 means "score only": no text,
 * global_abpoa.rs:241; modes 4, 5, 8, 9 take no seq_name — main.rs:260,268,311 hand the 0-based i to write_gaf only —
 * and every read gets its record whatever the index).  One thread at a time may call rg_stream_next on a stream.
 *
 * Memory: by default the stream holds whatever was pushed and not yet delivered (like the reference holds its whole
 * `sequences` vector, main.rs:24).  For read sets that do not fit, bound it: `max_queued_tiles` makes rg_stream_push /
 * rg_stream_feed_fasta wait while that many tiles sit in the queue, `max_undelivered_bytes` makes the workers wait
 * before they start another tile while finished tiles that rg_stream_next has not taken yet hold more than that (the
 * tile rg_stream_next is waiting for is always started: no deadlock), rg_stream_feed_fasta takes the FASTA text in
 * pieces, and rg_stream_release returns a kept record handle early.  With a bound the pushing and the consuming side
 * must be different threads, or one thread that drains with rg_stream_next whenever rg_stream_pending says so.
 */
typedef struct rg_stream rg_stream;
typedef struct rg_stream_opts {
    int32_t handles_per_device;   /* 0: default (3)                                                            */
    int32_t tile_reads;           /* 0: default (4096 in the pathwise modes, 8192 in the POA modes)            */
    int32_t format_threads;       /* host threads that format one tile; 0: default (hardware threads / workers, 1..16) */
    int32_t keep_records;         /* 1: every tile also keeps its records (rg_stream_result.records)           */
    int64_t seq_index_base;       /* seq_index of the first read pushed                                        */
    int32_t no_text;              /* 1: skip the GAF text (records only)                                       */
    int32_t spin_wait;            /* 0: the long waits for the device (one per kernel pipeline) poll an event with short
                                     sleeps — every HIP wait spins a CPU by default, 3 threads per GPU here, which a
                                     node under a CPU quota cannot afford; 1: hipStreamSynchronize for the handles of
                                     THIS stream (rg_set_option("spin_wait", 1) is the process-wide switch)      */
    int32_t max_queued_tiles;     /* > 0: pushes wait while this many tiles are queued (not yet taken by a handle) */
    int32_t amb_strand;           /* 1: `-s true` (main.rs:82-106, 132-165, 188-212, 229-253; POA modes, ignored in the
                                     others like main.rs:254-313 ignores it): the reads that qualify (global modes: score
                                     < 0; local modes: all) are aligned again, reverse-complemented, on a second handle of
                                     the same worker (scalar exec + reversed handle labels as in the reference), the
                                     reference's per-mode comparison picks the record, and the warning lines of both
                                     exec calls come before it.  Not together with keep_records.
                                     2: the same for a POA stream; for a stream of a pathwise mode it sets
                                     RG_AMB_BOTH_STRANDS on the stream's handles (our extension, see there; the kept
                                     record is the chosen one, so keep_records is fine)
                                     3: as 2, and on a pathwise stream RG_AMB_STRAND_VOTE as well
                                     Modes 26, 27 and 32 align both strands whatever this field says: 0, 1 and 2 give
                                     their exact rule, 3 the vote in modes 26 and 27 and RG_ERR_ARG in mode 32           */
    int64_t max_undelivered_bytes;/* > 0: see "Memory" above                                                     */
} rg_stream_opts;
typedef struct rg_stream_result {
    int64_t first_read;           /* index (push order) of the tile's first read                               */
    int64_t nreads;
    const char* text;             /* GAF text of the tile's reads in input order, NUL-terminated               */
    int64_t text_len;
    const int64_t* text_off;      /* nreads + 1: the text of read i is text[text_off[i] .. text_off[i + 1])      */
    const uint32_t* status;       /* nreads: RG_READ_* bits                                                    */
    const int32_t* score;         /* nreads: rg_result_score                                                   */
    int32_t device;               /* HIP device that aligned the tile                                          */
    int32_t reserved;
    uint64_t cell_updates;        /* DP cell updates of the tile (SURVEY 8d unit of work)                       */
    rg_batch* records;            /* keep_records: results-only handle for the rg_result_* accessors, owned by the
                                     stream (valid until rg_stream_release / rg_stream_destroy), else NULL      */
    uint64_t cell_updates_performed; /* rg_batch_cell_updates_performed of the tile                              */
} rg_stream_result;
#define RG_STREAM_END 1
void rg_stream_opts_default(rg_stream_opts* o);
int32_t rg_stream_create(const rg_graph* g, const rg_params* p, const int32_t* device_ids, int32_t ndev,
                         const rg_stream_opts* opts, rg_stream** out);
int32_t rg_stream_push(rg_stream* s, const char* reads, const int64_t* read_off, int64_t nreads, const char* const* names);
/* rg_reads_from_fasta + rg_stream_push in one pass: every time tile_reads more reads are complete they are pushed, so the
 * devices start while the rest of the text is parsed.  *nreads_out: reads pushed.  A text whose name / sequence counts
 * differ at its end returns RG_ERR_ARG ("wrong fasta file format", sequences.rs:41-43) AFTER the complete reads before
 * that point were pushed: the caller drops the stream. */
int32_t rg_stream_push_fasta(rg_stream* s, const char* fasta_text, int64_t len, int64_t* nreads_out);
/* The same for a text that arrives in pieces (a file read block by block: the reference's BufReader, sequences.rs:7):
 * any split is fine, even inside a line; what a piece leaves unfinished stays inside the stream.  final != 0 closes the
 * text (the name / sequence count check happens there).  *nreads_out: reads completed and pushed by THIS call.  One
 * FASTA text per stream at a time; rg_stream_push_fasta is feed(text, final = 1). */
int32_t rg_stream_feed_fasta(rg_stream* s, const char* piece, int64_t len, int32_t final, int64_t* nreads_out);
/* Tiles pushed and not yet delivered by rg_stream_next (queued + on a device + finished). */
int64_t rg_stream_pending(rg_stream* s);
/* keep_records: gives a tile's record handle back before rg_stream_destroy (the handle is freed). */
void rg_stream_release(rg_stream* s, rg_batch* records);
int32_t rg_stream_finish(rg_stream* s);
/* Error exit of a bounded stream (the caller's counterpart of a panic inside the reference's read loop, main.rs:56-105):
 * tiles still queued are dropped, every thread blocked in rg_stream_push / rg_stream_feed_fasta (waiting for room) or in
 * rg_stream_next returns RG_ERR_ARG ("stream aborted"), later calls fail the same way; the tiles on a device finish and
 * are discarded by rg_stream_destroy, which also waits for threads still inside a push / feed call.  Any thread. */
int32_t rg_stream_abort(rg_stream* s);
/* RG_OK: *out describes the next tile (pointers valid until the next rg_stream_next / rg_stream_destroy on this stream);
 * RG_STREAM_END: finished and everything delivered; negative: that tile failed. */
int32_t rg_stream_next(rg_stream* s, rg_stream_result* out);
void rg_stream_destroy(rg_stream* s);
/* Measurement hooks (bench.py): per-kernel device time summed over every tile so far (HIP events on the handles' own
 * streams; with several handles per device a kernel's time includes the other streams' kernels), the host phases
 * ("host:set_reads", "host:run", "host:fetch", "host:format": wall milliseconds summed over the worker threads and
 * tiles; "host:first_tile_create", "host:first_tile_run": the part of them spent on each handle's first tile, where
 * the handle is created and its HBM work buffers are allocated; "host:context_warmup": device context creation in the
 * worker threads at rg_stream_create) listed after the kernels, tiles done, handles that aligned a tile. */
int32_t rg_stream_kernel_count(rg_stream* s);
const char* rg_stream_kernel_name(rg_stream* s, int32_t k);
double rg_stream_kernel_ms(rg_stream* s, int32_t k);
int64_t rg_stream_kernel_launches(rg_stream* s, int32_t k);
int64_t rg_stream_tiles_done(rg_stream* s);
int32_t rg_stream_handles(rg_stream* s);      /* batch handles that aligned at least one tile */

/* Process-wide diagnostic switches, also settable through the environment (read once, before the first use).  The one table
 * they come from is RG_OPTIONS in recgraph_amd/csrc/rg_host.hpp; a switch takes 0 / 1 (any other value sets 1), an integer is
 * clamped to its range:
 *   "sweep_i32" (RG_SWEEP_I32: i32 sweep kernel even when the packed 16-bit one is admissible), "three_sweeps"
 *   (RG_THREE_SWEEPS), "no_frec" (RG_NO_FREC: Cand-list forward emission), "debug" (RG_DEBUG: list statistics on stderr; the
 *   packed k_opt0 is cross-checked against its i32 form), "spin_wait" (RG_SPIN_WAIT: hipStreamSynchronize instead of
 *   sleep-polling for the long waits), "no_gather" / "no_split" (RG_NO_GATHER / RG_NO_SPLIT: k_sweep16 without its gather runs /
 *   on the plain step tables), "no_spec" (RG_NO_SPEC: forward sweep pruned with the provable bound instead of the speculative
 *   one), "spec_margin" (RG_SPEC_MARGIN, -2^24..2^24, default 112: what the speculative bound subtracts from the picked path's
 *   score), "spec4_margin_x10" (RG_SPEC4_MARGIN_X10, 0..1000, default 25: ten times the factor -m 4 puts on that margin),
 *   "stripe_c" (RG_STRIPE_C, 0..32: 8, 16 or 32 columns per lane for reads longer than 2047 bases; 0 = 16 up to 8191 bases, 32
 *   beyond), "no_retire" (RG_NO_RETIRE, 0..3: 1 = k_sweep16 computes every path to the end; 2 / 3: retirement in the forward /
 *   reverse sweep only), "retire_shift" (RG_RETIRE_SHIFT, 2..12, default 8: the sweeps look for hopeless paths every 2^k step
 *   records; read when a handle builds its step tables — the test suite runs its small graphs at 4), "no_order" (RG_NO_ORDER:
 *   the sweeps' waves in read order instead of longest first), "dsel_edge" (RG_DSEL_EDGE, 1..2^20, default 8: the 1 / dsel_edge
 *   of the rows a sweep visits first always store their direction words), "no_dsel" (RG_NO_DSEL: every record of the packed
 *   sweeps stores its direction word, not only those with a picked path), "no_pick2" (RG_NO_PICK2: the speculative bound from
 *   one-path picks only), "layer_i32" (RG_LAYER_I32: the layer rebuild in its i32 form), "lds_pad" (RG_LDS_PAD, 0..40960 bytes,
 *   experiments only: extra dynamic LDS per k_sweep16 workgroup, which lowers the waves per CU), "chunk_reads" (RG_CHUNK_READS,
 *   0..2^20: most reads one launch of a DP kernel takes, in the pathwise and in the POA modes; 0 = what the memory budget allows), "launch_log" (RG_LAUNCH_LOG: every
 *   kernel launch of a batch leaves a pseudo-entry "inst:<instantiation>" in rg_batch_kernel_* / rg_stream_kernel_* — the
 *   demangled kernel name with its template arguments, e.g. "inst:rg::k_sweep16<16, 0, true, false, false>", ms 0, launches
 *   counted; off: no such entry), "layer_window" (RG_LAYER_WINDOW, 0..256, default 256: columns of the window the traceback layers
 *   of the packed pathwise modes are rebuilt in — 256, 128 (values in between count as 128), below 128: full rows; a read whose
 *   walk leaves the window is rebuilt at full width in the same batch and counted in the pseudo-entry "mem:layer_full_reads";
 *   the windowed kernel that ran is named by a pseudo-entry "mem:layer_window:<instantiation>", ms 0, launches counted).
 * The variants compute the same records byte for byte (tests/test_gpu_pathwise.py). */
int32_t rg_set_option(const char* name, int64_t value);
int64_t rg_get_option(const char* name);      /* -1: unknown option */

const char* rg_last_error(void);
int32_t rg_device_count(void);
int32_t rg_set_device(int32_t dev);

#ifdef __cplusplus
}
#endif
#endif
