// Host check of layer_window_left (recgraph_amd/csrc/layer_window/rg_layer_window.hpp), the one statement of where the column window
// of a layer row lies: for reads of n bases, EVERY start cell (layer row t_start, column start_col) and both window widths, over
// all the layer rows 0 .. t_start the walk can visit:
//   * the left edge is a multiple of the column-block width CW (and of 4, a byte of the layer buffer),
//   * it is monotone in t and moves by at most 4 columns per row,
//   * it lies inside [0, wpad - W],
//   * the start cell lies inside the window of its own row.
// Also layer_row_index against a linear search.
#include <cstdio>
#include <vector>

#include "layer_window/rg_layer_window.hpp"

int main() {
    const int ns[] = {1, 63, 255, 256, 1000, 1023};
    long long checked = 0;
    for (int n : ns) {
        int C = 4;
        while (C * 64 < n + 1) C *= 2;
        const int wpad = C * 64;
        for (int W : {rg::LAYER_WINDOW_NARROW, rg::LAYER_WINDOW_DEFAULT}) {
            const int CW = W / 64;
            const int rows = n + 70;                      // paths a little longer than the read
            for (int start_col = 0; start_col <= n; ++start_col)
                for (int t_start = 1; t_start <= rows; ++t_start) {
                    // left() reads (start_col - t_start) + t only: the rows of a start cell are the last rows of the start cell one step down
                    // its diagonal, so the row loop runs for the last start cell of every diagonal and every other one checks its own row
                    const bool last_of_diagonal = t_start == rows || start_col == n;
                    int prev = -1;
                    for (int t = last_of_diagonal ? 0 : t_start; t <= t_start; ++t) {
                        const int e = rg::layer_window_left(start_col, t_start, t, W, wpad);
                        if (e % CW || e % 4 || e < 0 || e > wpad - W || (prev >= 0 && (e < prev || e > prev + 4))) {
                            printf("n %d W %d start (%d, %d) t %d: left %d after %d\n", n, W, t_start, start_col, t, e, prev);
                            return 1;
                        }
                        prev = e;
                        ++checked;
                    }
                    if (start_col < prev || start_col >= prev + W) {
                        printf("n %d W %d: start cell (%d, %d) outside its window at %d\n", n, W, t_start, start_col, prev);
                        return 1;
                    }
                }
        }
    }
    for (int desc = 0; desc < 2; ++desc) {
        std::vector<int> list;
        for (int i = 0; i < 37; ++i) list.push_back(desc ? 1000 - 3 * i - (i % 2) : 5 + 3 * i + (i % 2));
        for (int row = 0; row < 1100; ++row) {
            int want = -1;
            for (int i = 0; i < (int)list.size(); ++i) if (list[i] == row) want = i;
            if (rg::layer_row_index(list.data(), (int)list.size(), row, desc != 0) != want) { printf("row index of %d\n", row); return 1; }
        }
    }
    printf("layer window ok (%lld rows)\n", checked);
    return 0;
}
