"""What the API and the CLI answer to both_strands / strand_vote in every mode the CLI admits: the text that
tests/golden/gap_mode_flag_refusals.txt records (tests/test_gap_mode_table_cpu.py compares byte for byte), and for the edit-distance
modes, with the CLI's answer to three scorings, tests/golden/edit_mode_flag_refusals.txt (tests/test_edit_mode_table_cpu.py)."""


def dump(modes, cli_check):
    """modes: the admitted `-m` values; cli_check(alignment_mode, both_strands, strand_vote, amb_strand): the CLI's flag validation
    (raises SystemExit, or returns whether `-s true` counts)."""
    from recgraph_amd import api
    out = []
    for mode in modes:
        for both in (False, True):
            for vote in (False, True):
                try:
                    res = "amb=%r" % api._both_strands_kw(mode, both, {}, vote).get("amb")
                except api._lib.RecGraphError as ex:
                    res = "error: %s" % ex
                out.append("api %d both=%d vote=%d -> %s\n" % (mode, both, vote, res))
                for amb_strand in ("false", "true"):
                    try:
                        res = "ok amb=%d" % bool(cli_check(mode, both, vote, amb_strand))
                    except SystemExit as ex:
                        res = str(ex)
                    out.append("cli %d both=%d vote=%d -s %s -> %s\n" % (mode, both, vote, amb_strand, res))
    return "".join(out)


def dump_edit_scores(modes, cli_check):
    """cli_check(alignment_mode, scores, gap_open, gap_extension): the CLI's scoring validation of the edit-distance modes (raises
    SystemExit, or returns), asked for the unit costs, the default scores and a 0 / -1 matrix without `-O 0 -E 1`; -O / -E as given."""
    from recgraph_amd import api
    unit, default = api.create_score_matrix_i32(0, -1), api.create_score_matrix_i32(2, -4)
    out = []
    for mode in modes:
        for name, scores, o, e in (("unit", unit, 0, 1), ("default", default, 4, 2), ("matrix", unit, 4, 2)):
            try:
                res = "ok %r" % cli_check(mode, scores, o, e)
            except SystemExit as ex:
                res = str(ex)
            out.append("cli scores %d %s -O %d -E %d -> %s\n" % (mode, name, o, e, res))
    return "".join(out)
