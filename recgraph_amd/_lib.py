"""ctypes binding of librecgraph_hip.so (the C ABI declared in include/recgraph_hip.h)."""
import collections
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# RG_LIB_PATH: another build of the same library (the statistics and retire-shift builds of tools/sweep_variants.sh); never set in tests
_SO = os.environ.get("RG_LIB_PATH") or os.path.join(_HERE, "librecgraph_hip.so")


class RecGraphError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"recgraph_hip error {code}: {msg}")
        self.code = code


class GafFields(C.Structure):
    _fields_ = [("has_record", C.c_int32), ("empty", C.c_int32), ("warning", C.c_uint32), ("strand", C.c_char),
                ("query_length", C.c_uint64), ("query_start", C.c_uint64), ("query_end", C.c_uint64),
                ("path_length", C.c_uint64), ("path_start", C.c_uint64), ("path_end", C.c_uint64),
                ("residue_matches_number", C.c_uint64), ("n_path_ids", C.c_int64), ("comments_len", C.c_int64)]


class StreamOpts(C.Structure):
    _fields_ = [("handles_per_device", C.c_int32), ("tile_reads", C.c_int32), ("format_threads", C.c_int32),
                ("keep_records", C.c_int32), ("seq_index_base", C.c_int64), ("no_text", C.c_int32), ("spin_wait", C.c_int32),
                ("max_queued_tiles", C.c_int32), ("amb_strand", C.c_int32), ("max_undelivered_bytes", C.c_int64)]


class StreamResult(C.Structure):
    _fields_ = [("first_read", C.c_int64), ("nreads", C.c_int64), ("text", C.c_void_p), ("text_len", C.c_int64),
                ("text_off", C.POINTER(C.c_int64)), ("status", C.POINTER(C.c_uint32)), ("score", C.POINTER(C.c_int32)),
                ("device", C.c_int32), ("reserved", C.c_int32), ("cell_updates", C.c_uint64), ("records", C.c_void_p),
                ("cell_updates_performed", C.c_uint64)]


class Params(C.Structure):
    _fields_ = [("mode", C.c_int32), ("scores", C.c_int32 * 36), ("gap_open", C.c_int32), ("gap_ext", C.c_int32),
                ("band_b", C.c_float), ("band_f", C.c_float), ("bta_override", C.c_int64),
                ("base_rec_cost", C.c_int32), ("multi_rec_cost", C.c_float), ("rec_band_width", C.c_float),
                ("amb_mode", C.c_int32)]


AMB_BOTH_STRANDS = 4     # RG_AMB_BOTH_STRANDS (include/recgraph_hip.h): bit 2 of Params.amb_mode, pathwise modes
AMB_STRAND_VOTE = 8      # RG_AMB_STRAND_VOTE: bit 3, only together with bit 2 — the first strand by a 12-mer vote

# The affine-gap pathwise modes (values of Params.mode, no entry points of their own): a rule in a family, `mode = the rule's base mode +
# the family's offset`.  The rows of csrc/rg_gap_modes.hpp once more, with the fixed text of the Python side's refusals; DESIGN 4.8 has
# the table in words.  From it come the MODE_PATHWISE_GAP_* names here and in api, api's tuples and flag rules, and the CLI's.
GAP_RULES = (("", 6), ("_SEMI", 7), ("_LOCAL", 12))      # (infix of the name, base mode): global, semiglobal, local
GAP_GLOBAL, GAP_SEMI, GAP_LOCAL = 0, 1, 2                # indices into GAP_RULES
GapFamily = collections.namedtuple("GapFamily", "suffix offset max_stripes both_strands one_stripe_dirs staged api_refusal cli_refusal "
                                                "cli_refusal_local cli_help")
# max_stripes: the longest read is max_stripes * 2048 - 1 bases; both_strands: the mode itself says both strands (the flag is redundant,
# the vote a rule of the global and semiglobal modes), otherwise the reads are aligned as given and both flags are refused: api_refusal
# (%s: the flag), cli_refusal (cli_refusal_local: what the local mode says instead); one_stripe_dirs: the checkpointed traceback;
# staged: two PICK stages and one TRACE stage instead of two passes
_AS_GIVEN = "%s is not available in the affine-gap pathwise modes (6, 7, 12 and their long-read flavours 16, 17, 22)"
_CLI_AS_GIVEN = "--both-strands / --strand-vote are not available in mode%s: %s the reads as given"
GAP_FAMILIES = (
    GapFamily("", 0, 1, False, False, False, _AS_GIVEN, _CLI_AS_GIVEN % ("s 6 and 7", "they align"), _CLI_AS_GIVEN % (" 12", "it aligns"),
              "12: local affine-gap pathwise"),
    GapFamily("_LONG", 10, 8, False, False, False, _AS_GIVEN, _CLI_AS_GIVEN % ("s 16, 17 and 22", "they align"), None,
              "16, 17, 22: modes 6, 7, 12 for reads of up to 16383 bases"),
    GapFamily("_STRANDS", 20, 8, True, False, False, None, None, None,
              "26, 27, 32: those on both strands (--strand-vote: 26 and 27 only)"),
    GapFamily("_XLONG", 50, 64, False, True, False,
              "%s is not available in the affine-gap pathwise modes for reads of up to 131071 bases (56, 57, 62): they align the reads as given",
              _CLI_AS_GIVEN % ("s 56, 57 and 62", "they align"), None,
              "56, 57, 62: modes 6, 7, 12 for reads of up to 131071 bases"),
    GapFamily("_XSTRANDS", 70, 64, True, True, True, None, None, None,
              "76, 77, 82: those on both strands, the traceback run once, on the strand that won (--strand-vote: 76 and 77 only)"),
)
GapMode = collections.namedtuple("GapMode", "rule family")      # rule: GAP_GLOBAL / GAP_SEMI / GAP_LOCAL
_GAP_MODES = {base + f.offset: GapMode(r, f) for f in GAP_FAMILIES for r, (_, base) in enumerate(GAP_RULES)}
GAP_MODE_NAMES = {"MODE_PATHWISE_GAP%s%s" % (GAP_RULES[m.rule][0], m.family.suffix): mode for mode, m in _GAP_MODES.items()}
globals().update(GAP_MODE_NAMES)      # MODE_PATHWISE_GAP = 6 ... MODE_PATHWISE_GAP_LOCAL_XSTRANDS = 82 (RG_MODE_* in include/recgraph_hip.h)


def gap_mode(mode):
    """GapMode(rule, family) of an affine-gap pathwise mode, None for every other value."""
    return _GAP_MODES.get(mode)


def gap_family(suffix):
    return next(f for f in GAP_FAMILIES if f.suffix == suffix)


def gap_family_modes(*suffixes):
    """The modes of the named families, family by family, each in the order global, semiglobal, local."""
    return tuple(base + gap_family(s).offset for s in suffixes for _, base in GAP_RULES)


# The bit-vector edit-distance pathwise modes (values of Params.mode, no entry points of their own): a rule in a family, `mode = the
# rule's base mode + the family's offset`, each family a family of the table above restricted to unit costs.  The rows of
# csrc/rg_edit_modes.hpp once more, with the fixed text of the Python side's refusals; DESIGN 4.14 has the table in words.  From it come
# the MODE_PATHWISE_EDIT* names here and in api, api's tuples and flag rule, and the CLI's.  No rows of the table above: gap_mode(44) is None.
EDIT_RULES = (("", 44), ("_SEMI", 45))      # (infix of the name, base mode): global, semiglobal
EditFamily = collections.namedtuple("EditFamily", "suffix offset max_read gap_suffix score_refusal api_refusal cli_refusal cli_help")
# max_read: the longest read, in bases; gap_suffix: the family of GAP_FAMILIES whose rule, bytes and read limit these are at unit costs;
# score_refusal: what the CLI says to any other scoring; api_refusal (%s: the flag), cli_refusal: the reads are aligned as given
_EDIT_SCORES = ("the edit-distance pathwise modes (%s) take unit costs only: -M 0 -X 1 -O 0 -E 1, or a -t matrix whose ACGTN x ACGTN "
                "entries are all 0 or -1 with -O 0 -E 1; every other scoring is what %s are for")
EDIT_FAMILIES = (
    EditFamily("", 0, 16383, "_LONG", _EDIT_SCORES % ("-m 44 / -m 45", "-m 16 / -m 17"),
               "%s is not available in the edit-distance pathwise modes (44, 45): they align the reads as given",
               _CLI_AS_GIVEN % ("s 44 and 45", "they align"),
               "44, 45: modes 16, 17 at unit costs (-M 0 -X 1 -O 0 -E 1 must be given) on the bit-vector kernels"),
    EditFamily("_XLONG", 50, 131071, "_XLONG", _EDIT_SCORES % ("-m 94 / -m 95", "-m 56 / -m 57"),
               "%s is not available in the edit-distance pathwise modes for reads of up to 131071 bases (94, 95): they align the reads as given",
               _CLI_AS_GIVEN % ("s 94 and 95", "they align"),
               "94, 95: those for reads of up to 131071 bases (modes 56, 57 at unit costs)"),
)
EditMode = collections.namedtuple("EditMode", "semi family")
_EDIT_MODES = {base + f.offset: EditMode(bool(r), f) for f in EDIT_FAMILIES for r, (_, base) in enumerate(EDIT_RULES)}
EDIT_MODE_NAMES = {"MODE_PATHWISE_EDIT%s%s" % (EDIT_RULES[m.semi][0], m.family.suffix): mode for mode, m in _EDIT_MODES.items()}
globals().update(EDIT_MODE_NAMES)      # MODE_PATHWISE_EDIT = 44 ... MODE_PATHWISE_EDIT_SEMI_XLONG = 95 (RG_MODE_* in include/recgraph_hip.h)


def edit_mode(mode):
    """EditMode(semi, family) of an edit-distance pathwise mode, None for every other value."""
    return _EDIT_MODES.get(mode)


def edit_family_modes(suffix):
    """The modes of the named family: global, semiglobal."""
    return tuple(mode for mode, m in _EDIT_MODES.items() if m.family.suffix == suffix)


# The two both-strands edit-distance pathwise modes (csrc/rg_edit_strands_modes.hpp; RG_MODE_PATHWISE_EDIT_STRANDS in
# include/recgraph_hip.h): modes 44 / 45 with both strands of every read scored in one wave.  Deliberately NO rows of EDIT_FAMILIES or
# GAP_FAMILIES: edit_mode(64) and gap_mode(64) are None, and EDIT_MODE_NAMES stays as it is — the flag rule (both strands is the mode
# itself, the vote is refused) is that of no row there.
EDIT_STRANDS_MODES = (64, 65)               # global, semiglobal: the rules of modes 26 / 27 at unit costs
EDIT_STRANDS_MAX_READ = 16383
EDIT_STRANDS_MODE_NAMES = {"MODE_PATHWISE_EDIT_STRANDS": 64, "MODE_PATHWISE_EDIT_SEMI_STRANDS": 65}
globals().update(EDIT_STRANDS_MODE_NAMES)
EDIT_STRANDS_SCORE_REFUSAL = ("the both-strands edit-distance pathwise modes (-m 64 / -m 65) take unit costs only: -M 0 -X 1 -O 0 -E 1, or a -t "
                              "matrix whose ACGTN x ACGTN entries are all 0 or -1 with -O 0 -E 1; every other scoring is what -m 26 / -m 27 are for")
EDIT_STRANDS_VOTE_REFUSAL = ("%s is not available in the both-strands edit-distance pathwise modes (64, 65): both strands of every read "
                             "are scored in one pass, so a 12-mer vote would save nothing and would change the rule")
EDIT_STRANDS_CLI_HELP = "64, 65: modes 44, 45 on both strands, scored in one pass and traced once (modes 26, 27 at unit costs)"


def edit_strands_mode(mode):
    """``semi`` (False / True) of a both-strands edit-distance pathwise mode, None for every other value."""
    return bool(EDIT_STRANDS_MODES.index(mode)) if mode in EDIT_STRANDS_MODES else None


def unit_costs(table, gap_open, gap_ext):
    """What every edit-distance mode admits: gap_open 0, gap_ext -1 and a 36-entry score table whose ACGTN x ACGTN block holds 0 and -1 only."""
    return gap_open == 0 and gap_ext == -1 and all(table[a * 6 + b] in (0, -1) for a in range(5) for b in range(5))


READ_UNALIGNED = 16     # RG_READ_UNALIGNED: status bit of that mode — the read has no local alignment, and no record


def library_path():
    return _SO


def build_library(force=False):
    """Compile every HIP source for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return _SO


# every symbol include/recgraph_hip.h declares
SYMBOLS = ["rg_params_default", "rg_scores_match_mis", "rg_graph_from_gfa", "rg_graph_create_lnz",
           "rg_graph_create_path", "rg_graph_destroy", "rg_graph_path_error", "rg_graph_rows", "rg_graph_paths", "rg_graph_dump",
           "rg_batch_create", "rg_batch_set_reads", "rg_batch_run", "rg_batch_fetch", "rg_batch_destroy", "rg_batch_size",
           "rg_result_status", "rg_result_score", "rg_result_gaf", "rg_result_fields", "rg_batch_format_all", "rg_batch_cell_updates", "rg_batch_cell_updates_performed", "rg_batch_kernel_count",
           "rg_batch_kernel_name", "rg_batch_kernel_ms", "rg_batch_kernel_launches", "rg_align_batch", "rg_align_batch_multi", "rg_multi_shards", "rg_multi_batch", "rg_multi_shard_begin",
           "rg_multi_format_all", "rg_multi_destroy", "rg_last_error",
           "rg_device_count", "rg_set_device",
           "rg_reads_from_fasta", "rg_reads_count", "rg_reads_bases", "rg_reads_offsets", "rg_reads_names", "rg_reads_destroy", "rg_fasta_check",
           "rg_stream_opts_default", "rg_stream_create", "rg_stream_push", "rg_stream_push_fasta", "rg_stream_feed_fasta", "rg_stream_pending",
           "rg_stream_release", "rg_stream_finish", "rg_stream_abort", "rg_stream_next",
           "rg_stream_destroy", "rg_stream_kernel_count", "rg_stream_kernel_name", "rg_stream_kernel_ms",
           "rg_stream_kernel_launches", "rg_stream_tiles_done", "rg_stream_handles", "rg_set_option", "rg_get_option"]

_lib = None


def load():
    """Load the HIP library; fails loudly when it has not been built (there is no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise RecGraphError(-3, f"{_SO} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(the product has no CPU fallback)")
    l = C.CDLL(_SO)
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    P = C.POINTER
    l.rg_params_default.argtypes = [P(Params), i32]
    l.rg_scores_match_mis.argtypes = [i32, i32, i32, P(i32)]
    l.rg_graph_from_gfa.argtypes = [C.c_char_p, i64, P(vp)]
    l.rg_graph_create_lnz.argtypes = [C.c_char_p, i64, P(i64), P(i64), P(u64), P(vp)]
    l.rg_graph_create_path.argtypes = [C.c_char_p, i64, i32, P(u64), P(i64), P(i64), P(u64), P(u64), P(vp)]
    l.rg_graph_destroy.argtypes = [vp]
    l.rg_graph_path_error.argtypes = [vp]
    l.rg_graph_path_error.restype = C.c_char_p
    l.rg_graph_rows.argtypes = [vp]
    l.rg_graph_rows.restype = i64
    l.rg_graph_paths.argtypes = [vp]
    l.rg_graph_dump.argtypes = [vp, i32, C.c_char_p, i64]
    l.rg_graph_dump.restype = i64
    l.rg_batch_create.argtypes = [vp, P(Params), C.c_char_p, P(i64), i64, P(vp)]
    l.rg_batch_set_reads.argtypes = [vp, C.c_char_p, P(i64), i64]
    l.rg_align_batch.argtypes = [vp, P(Params), C.c_char_p, P(i64), i64, P(vp)]
    for f in ("rg_batch_run", "rg_batch_fetch"):
        getattr(l, f).argtypes = [vp]
    l.rg_batch_destroy.argtypes = [vp]
    l.rg_batch_size.argtypes = [vp]
    l.rg_batch_size.restype = i64
    l.rg_result_status.argtypes = [vp, i64]
    l.rg_result_status.restype = C.c_uint32
    l.rg_result_score.argtypes = [vp, i64]
    l.rg_result_gaf.argtypes = [vp, i64, C.c_char_p, i64, C.c_char_p, i64]
    l.rg_result_gaf.restype = i64
    l.rg_result_fields.argtypes = [vp, i64, P(GafFields), P(u64), i64, C.c_char_p, i64]
    l.rg_align_batch_multi.argtypes = [vp, P(Params), C.c_char_p, P(i64), i64, P(i32), i32, P(vp)]
    l.rg_multi_shards.argtypes = [vp]
    l.rg_multi_batch.argtypes = [vp, i32]
    l.rg_multi_batch.restype = vp
    l.rg_multi_shard_begin.argtypes = [vp, i32]
    l.rg_multi_shard_begin.restype = i64
    l.rg_multi_format_all.argtypes = [vp, P(C.c_char_p), i64, C.c_char_p, i64, i32]
    l.rg_multi_format_all.restype = i64
    l.rg_multi_destroy.argtypes = [vp]
    l.rg_batch_format_all.argtypes = [vp, P(C.c_char_p), i64, C.c_char_p, i64, i32]
    l.rg_batch_format_all.restype = i64
    l.rg_batch_cell_updates.argtypes = [vp]
    l.rg_batch_cell_updates.restype = u64
    l.rg_batch_cell_updates_performed.argtypes = [vp]
    l.rg_batch_cell_updates_performed.restype = u64
    l.rg_batch_kernel_count.argtypes = [vp]
    l.rg_batch_kernel_name.argtypes = [vp, i32]
    l.rg_batch_kernel_name.restype = C.c_char_p
    l.rg_batch_kernel_ms.argtypes = [vp, i32]
    l.rg_batch_kernel_ms.restype = C.c_double
    l.rg_batch_kernel_launches.argtypes = [vp, i32]
    l.rg_batch_kernel_launches.restype = i64
    l.rg_last_error.restype = C.c_char_p
    l.rg_set_device.argtypes = [i32]
    l.rg_reads_from_fasta.argtypes = [C.c_char_p, i64, P(vp)]
    l.rg_reads_count.argtypes = [vp]
    l.rg_reads_count.restype = i64
    l.rg_reads_bases.argtypes = [vp]
    l.rg_reads_bases.restype = vp
    l.rg_reads_offsets.argtypes = [vp]
    l.rg_reads_offsets.restype = P(i64)
    l.rg_reads_names.argtypes = [vp]
    l.rg_reads_names.restype = P(C.c_char_p)
    l.rg_reads_destroy.argtypes = [vp]
    l.rg_fasta_check.argtypes = [C.c_char_p, i64, i32, P(i64), P(i64)]
    l.rg_stream_opts_default.argtypes = [P(StreamOpts)]
    l.rg_stream_create.argtypes = [vp, P(Params), P(i32), i32, P(StreamOpts), P(vp)]
    l.rg_stream_push.argtypes = [vp, vp, P(i64), i64, P(C.c_char_p)]
    l.rg_stream_push_fasta.argtypes = [vp, C.c_char_p, i64, P(i64)]
    l.rg_stream_feed_fasta.argtypes = [vp, C.c_char_p, i64, i32, P(i64)]
    l.rg_stream_pending.argtypes = [vp]
    l.rg_stream_pending.restype = i64
    l.rg_stream_release.argtypes = [vp, vp]
    l.rg_stream_release.restype = None
    l.rg_stream_finish.argtypes = [vp]
    l.rg_stream_abort.argtypes = [vp]
    l.rg_stream_next.argtypes = [vp, P(StreamResult)]
    l.rg_stream_destroy.argtypes = [vp]
    l.rg_stream_kernel_count.argtypes = [vp]
    l.rg_stream_kernel_name.argtypes = [vp, i32]
    l.rg_stream_kernel_name.restype = C.c_char_p
    l.rg_stream_kernel_ms.argtypes = [vp, i32]
    l.rg_stream_kernel_ms.restype = C.c_double
    l.rg_stream_kernel_launches.argtypes = [vp, i32]
    l.rg_stream_kernel_launches.restype = i64
    l.rg_stream_tiles_done.argtypes = [vp]
    l.rg_stream_tiles_done.restype = i64
    l.rg_stream_handles.argtypes = [vp]
    l.rg_set_option.argtypes = [C.c_char_p, i64]
    l.rg_get_option.argtypes = [C.c_char_p]
    l.rg_get_option.restype = i64
    _lib = l
    return l


def check(rc):
    if rc != 0:
        raise RecGraphError(rc, load().rg_last_error().decode())
