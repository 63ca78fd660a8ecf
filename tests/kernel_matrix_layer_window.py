"""The kernel matrix of recgraph_amd/csrc/layer_window/rg_layer_window.hip (the traceback layers inside a column window): one entry
per compiled `__global__` instantiation, as data — the contract of tests/kernel_matrix.py applied to a directory of its own, like
tests/kernel_matrix_gap.py.

MATRIX maps the name of an instantiation (what tools/kernel_resources.py report() prints and the launch log records as
"mem:layer_window:<name>", a pseudo-statistic that is always on — "inst:" entries are those of tests/kernel_matrix.py, which accounts for every one its cases log) to the id of a case of tests/test_gpu_layer_window.py that launches it.  tests/test_kernel_matrix_layer_window_cpu.py
checks that the key set equals what hipcc compiles; the GPU test runs every case, compares every read with the
oracle and with the same call at layer_window 0, and asserts that the entry's instantiation was launched.

k_layer_win<C, CW>: C columns per lane of the sweep that wrote the direction words (4: reads up to 255 bases, 8: up to 511, 16: up to
1023), CW columns per lane of the window (4: 256 columns, the default; 2: 128 columns)."""


def win(C, CW):
    return "rg::k_layer_win<%d, %d>" % (C, CW)


MATRIX = {
    win(4, 4): "short",          # reads of 100-255 bases, window 256: the window covers the row
    win(4, 2): "edges-128",      # -m 9 / -m 5 on short reads and reads of at most 127 bases, window 128
    win(8, 4): "edges-256",      # 300-base reads among the edge cases, window 256
    win(8, 2): "indels",         # 300-base reads with a 100-base deletion / insertion, window 128
    win(16, 4): "config5",       # 1000-base reads, window 256
    win(16, 2): "edges-128",     # the 1023-base read, window 128
}
CASES = sorted(set(MATRIX.values()))
