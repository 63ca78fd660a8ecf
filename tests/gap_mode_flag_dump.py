"""What the API and the CLI answer to both_strands / strand_vote in every mode the CLI admits: the text that
tests/golden/gap_mode_flag_refusals.txt records (tests/test_gap_mode_table_cpu.py compares byte for byte)."""


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
