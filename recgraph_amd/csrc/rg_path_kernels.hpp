// Argument blocks of the pathwise kernels (rg_pathwise.hip) shared with the driver.
#pragma once
#include "rg_path_args.hpp"
#include "rg_path_plan.hpp"      // ReadState, Cand
#include "rg_launch_log.hpp"
#include "layer_window/rg_layer_window.hpp"      // ST_LAYER_FULL, layer_window_left

namespace rg {

// Direction word of k_sweep16 at C <= 16 (RowOps16::dir_word, LayerArgs::dir_fmt 1) -> U and L as bit-per-column masks in the
// lane's column order (bit q = column q of the lane): register r of the packed row holds columns r and H + r and contributes
// bit 7 - r of byte 0 (U, column r), byte 1 (U, column H + r), byte 2 (L, column r), byte 3 (L, column H + r)
template <int H>
__device__ __forceinline__ void dir16_decode(unsigned w, unsigned& u16, unsigned& l16) {
    constexpr unsigned LOWH = (1u << H) - 1u;
    const unsigned t = __brev(w);
    u16 = ((t >> 24) & LOWH) | (((t >> 16) & LOWH) << H);
    l16 = ((t >> 8) & LOWH) | ((t & LOWH) << H);
}

struct SweepArgs {
    PathGraphDev g;
    DevScores sc;
    const uint8_t* reads;
    const long long* read_off;
    const uint8_t* bad;
    ReadState* state;
    int* roll;                 // [reads][P][wpad] rolling rows (packed pairs for k_sweep16: half the words)
    int rev;                   // 0 forward sweep, 1 reverse sweep
    int track_best;            // maintain the best member per (row, col) (m8)
    const int* thr;            // [reads][wpad] emission thresholds by real column, or null
    const int4* fsteps;        // step tables (one record per (row, edge group), sweep order), see k_sweep
    const int4* rsteps;
    int nfsteps, nrsteps;
    const int4* fsplit;        // the same records with TAILs (rg_path_driver.hip: split tables), or null; launch_sweep16 hands
    const int4* rsplit;        // them to the record variants of k_sweep16 when `use_split` says the batch qualifies
    int use_split;
    const int* lb;             // per read lower bound of S0: when set (forward sweep only) the threshold of column
                               // j is lb + brc - (n - j) * maxmatch (no reverse information needed)
    int brc, maxmatch;
    int semi;                  // semiglobal modes (-m 5 / -m 9): border column stays 0, free end row
    float rbw;                 // -B: columns outside the recombination band never emit
    int* colmax_out;           // [reads][wpad] per-column maximum of the best members, or null
    int* colarg_out;           // [reads][wpad] (row << 8 | path) of a cell attaining that maximum
    Cand* cand;                // [reads][cand_cap] or null
    unsigned cand_cap;         // capacity of the list this sweep appends to
    unsigned* ncand_out;
    uint32_t* dirs;            // [reads][dirs_stride] direction words or null
    long long dirs_stride;
    int dir_words;             // u32 words per (row, group) slot
    unsigned long long* cells;   // [2]: member-row cell updates of the workload | cell updates the kernel performed
    int count_cells;
    int oob;                   // 1: the thresholds are tight (speculative bound): the epilogue tests the lane maximum before the columns
    // k_sweep16, two-sweep pipeline: emissions go out as one record per (row, lane) instead of one Cand per cell: (4 + C) ints = {row << 6 | lane, column mask, 0, 0, key[C]} with key = value << 16 | path
    int* frec;                 // [reads][frec_cap][4 + C] or null
    unsigned frec_cap;
    int nwv;                   // waves (column stripes of 2048) per read: > 1 for reads longer than 2047 bases (k_sweep<32, true, true>)
    int gather_ok;             // k_sweep16 gather runs: the difference of two members' packed values provably fits 16 bits
    // k_sweep16 PATH RETIREMENT (record pipelines, P <= 64): per 256 records of the step table and per path, the union of the
    // member masks of the groups the path leads from there on ([evaluation point][64]); one table per step table.
    // Evaluation points: every 2^retire_shift records (StepTables::retire_shift: what the table builder used)
    const unsigned long long* flead;
    const unsigned long long* rlead;
    const unsigned long long* fslead;   // ... of the split tables
    const unsigned long long* rslead;
    int retire;
    int retire_shift;
    const int* order;                   // launch order of the reads (block b sweeps read order[b]) or null: see launch_order
    unsigned long long table_members;   // member rows of the step table in use (k_sweep16 with path retirement counts cells from it)
    unsigned long long fmembers, rmembers;
    // k_sweep16, DIRECTION WORDS ON DEMAND: the picks of k_pick (pick[rd]; pick2[2 rd] = second path or -1) — only the (row, group)
    // records with one of those paths among their members store a direction word; k_verify sends a read whose final paths are
    // not among them to the second pass.  Null: every record stores its word.
    const int* dsel_pick;
    const int* dsel_pick2;
    // ... and every record of the rows the sweep visits first (forward: rows < dsel_lo, reverse: rows > dsel_hi) stores its word
    // whatever its members: the reference's search likes to switch to another path for the last few columns of a read (ties
    // among the paths of a shared end segment go to the highest path id), and such a path's layer is only rebuilt over those rows
    int dsel_lo, dsel_hi;
    // k_sweep16, SILENT RUNS (narrow record variants): [8] rows of the silent register runs | rows of all register runs of the
    // launch | the six key counters (eager member folds | rows closed | rows that wrote a record | members left out of gather
    // pass (1) | of general-path folds | of silent-run tails) — words NEED_SILENT_ROWS .. NEED_KEY_SAVED_TAIL of the chunk's need[]
    // read-back — or null
    unsigned* runstat;
};
// words of the chunk's need[] read-back that count the rows of the silent runs and of all register runs of the record sweeps
// (0 .. 3: k_need, 4: k_verify, 5: NEED_LAYER_FULL); reported as "mem:silent_rows" / "mem:run_rows"
constexpr int NEED_SILENT_ROWS = 6;
constexpr int NEED_RUN_ROWS = 7;
// ... and the key work of the tails and general-path records of those sweeps (k_sweep16, KEY WORK THAT NO RECORD USES); reported as
// "mem:key_folds" / "mem:key_rows" / "mem:key_rows_hit" / "mem:key_folds_saved" (the sum of the three places) and
// "mem:key_saved_gather" / "mem:key_saved_general" / "mem:key_saved_tail"
constexpr int NEED_KEY_FOLDS = 8;
constexpr int NEED_KEY_ROWS = 9;
constexpr int NEED_KEY_ROWS_HIT = 10;
constexpr int NEED_KEY_SAVED_GATHER = 11;
constexpr int NEED_KEY_SAVED_GENERAL = 12;
constexpr int NEED_KEY_SAVED_TAIL = 13;
constexpr int NEED_WORDS = 14;      // (even: the read-back packs them into 64-bit words)

// expands the (row, lane) records of the forward sweep into Cand entries, keeping only cells that can still reach
// the final bound with the best reverse partner of their column
struct ExpandArgs {
    ReadState* state;
    const int* frec;           // records of this sweep
    unsigned frec_cap;
    const unsigned* nrec;
    Cand* fcand;               // out: Cand list of this sweep
    unsigned fcap;
    unsigned* nf;
    const int* wr;             // [reads][wpad] column maxima of the OTHER sweep (best possible partner per column)
    int wpad;
    int brc;
    const int* knm;            // per row: highest path id NOT through the row (-1 if none)
    int rev;                   // records of the reverse sweep: lane columns are mirrored (real column = n - c)
    const long long* read_off;
    float rbw;                 // -B
    int gcost;                 // uniform read-gap cost: the records hold z-space keys (z = A - c * gcost, rg_sweep16.hip)
};

struct SeedArgs {
    PathGraphDev g;
    ReadState* state;
    int nreads;
    int mode;
    DevScores sc;
    const uint8_t* reads;
    const long long* read_off;
};

struct ThrArgs {
    const ReadState* state;
    const int* colmax;
    int* thr;
    int wpad;
    int brc;
    int use_bound;             // 0: S0, 1: the tighter bound of k_bound
    const int* lb;             // the forward sweep's lower bound of the search maximum (or null): the base is at least that — with
                               // a two-path pick it lies above the seed; k_verify checks the speculative ones afterwards
};

struct BoundArgs {
    PathGraphDev g;
    ReadState* state;
    const long long* read_off;
    const int* mf; const int* mfarg;
    const int* wr; const int* wrarg;
    int wpad;
    int brc;
    float mrc;
    float rbw;
};

struct Opt0Args {
    PathGraphDev g;
    DevScores sc;
    const uint8_t* reads;
    const long long* read_off;
    const uint8_t* bad;
    const int* fpoff; const int* fprow;
    int* lb;                   // out: exact global alignment score of the read against path 0 (pick == null) ...
    int semi;
    const int* pick;           // ... or against path pick[rd], minus `margin`: the SPECULATIVE bound (see k_pick)
    int margin;
    int nwv;                   // column stripes per read (> 1: k_opt0_striped)
    const int* pick2;          // two-path picks {p2 or -1, X} (PickArgs), or null
    int rec_pen;               // what a two-path bound pays for its switch: base recombination cost + displacement allowance
};

// The rows the bound kernels walk for one read (k_opt0, k_opt0_striped; k_opt0_16 states the same walk with a two-stage look-ahead), and the bound they write: the rows of the picked
// path — path 0 without picks: only its score is a provable bound (PickArgs) — or, for a two-path pick, p1's rows up to X followed by
// p2's rows above X (both lists ascending; every wave of a striped read takes the same rows).  A walk is
//     for (int t = 0; t < pr.cnt; ++t) { if (!pr.row(t, i)) continue; ... }
// row() returns false for the one iteration that switches to p2's list and moves t in front of its first row above X.
struct PickedRows {
    const int* fpoff; const int* fprow;
    int pk, pk2, X, beg, cnt;
    bool second;
    __device__ __forceinline__ PickedRows(const Opt0Args& a, int rd) : fpoff(a.fpoff), fprow(a.fprow), second(false) {
        pk = a.pick ? a.pick[rd] : 0;
        pk2 = (a.pick && a.pick2) ? a.pick2[2 * rd] : -1;
        X = pk2 >= 0 ? a.pick2[2 * rd + 1] : INT32_MAX;
        beg = fpoff[pk]; cnt = fpoff[pk + 1] - beg;
    }
    // p2's list; -> index of its first row above X
    __device__ __forceinline__ int switch_lists() {
        second = true;
        beg = fpoff[pk2]; cnt = fpoff[pk2 + 1] - beg;
        int lo = 0, hi = cnt;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (fprow[beg + mid] <= X) lo = mid + 1; else hi = mid; }
        return lo;
    }
    __device__ __forceinline__ bool row(int& t, int& i) {
        i = fprow[beg + t];
        if (i > X && !second) { t = switch_lists() - 1; return false; }
        return true;
    }
    // lb[rd] from the walk's score: minus the margin of a speculative bound and what a two-path bound pays for its switch
    __device__ __forceinline__ void write_bound(const Opt0Args& a, int rd, int score) const {
        a.lb[rd] = score - (a.pick ? a.margin : 0) - (pk2 >= 0 ? a.rec_pen : 0);
    }
};

// Speculative lower bound of the -m 8 search maximum.  The forward sweep of the two-sweep pipeline emits every cell that
// could still pair up to `lb`; the only PROVABLE lb before the sweep is the alignment of the read against path 0 (the one
// path that is the alpha of all its groups), which lies ~1500 below the seed at config 5 and lets 40 000 records per read
// through.  Instead: k_pick votes for the path that shares most sampled 12-mers with the read, k_opt0 aligns the read
// against THAT path, lb' = that score - margin, and k_verify checks the speculation afterwards: the pruning with lb' is
// exact iff the search maximum found is >= lb' (every pair that beats or ties it was then kept); the reads that fail
// (rs->status & ST_RETRY) are aligned again with the provable bound (rg_path_driver.hip).
struct PickArgs {
    const uint8_t* reads;
    const long long* read_off;
    const uint8_t* bad;
    const uint32_t* keys;      // open-addressing table of the 12-mers of every path: key (24 bits) or 0xffffffff
    const unsigned long long* masks;   // paths that contain the 12-mer (P <= 64)
    unsigned table_mask;       // table size - 1 (power of two)
    int P;
    int* pick;                 // out: path with the most votes (lowest id on ties; 0 when nothing matched)
    // TWO-PATH PICK (reads that switch haplotype once: half of config 5).  The votes are per sample position, so the wave
    // also finds the split t and the paths (p1, p2) that maximise votes_{< t}(p1) + votes_{>= t}(p2); when that beats the
    // one-path vote clearly, pick2[rd] = {p2, X}: X = a row both paths visit near the split.  k_opt0 then aligns the read
    // against p1's rows <= X followed by p2's rows > X — the alignment a recombination p1 -> p2 behind the shared segment
    // realises — and the bound is that score minus the recombination cost.  Speculative like the one-path pick.
    const int* fpoff; const int* fprow;
    int* pick2;                // out (null: one-path picks only): {p2 or -1, X}
};
constexpr uint32_t ST_RETRY = 0x200u;   // internal: the speculative bound of this read did not hold

struct SearchArgs {
    PathGraphDev g;
    ReadState* state;
    const Cand* fcand;
    const Cand* rcand;
    const unsigned* nf;
    const unsigned* nr;
    unsigned* ridx;
    unsigned fcap, rcap;
    const int* wr;             // [reads][wpad] reverse column maxima: forward candidates are re-filtered with the
                               // final bound before pairing (they may have been emitted with the loose lb threshold)
    int wpad;
    int brc;
    float mrc;
};

struct LayerArgs {
    PathGraphDev g;
    DevScores sc;
    const uint8_t* reads;
    const long long* read_off;
    ReadState* state;
    int rev;
    const uint32_t* dirs;
    long long dirs_stride;
    int dir_words;
    int dir_fmt;               // 0: 2 bits per column (k_sweep), 1: U mask | L mask (k_sweep16)
    int semi;
    int* layer;                // [reads][layer_stride]: traceback decisions, (rows of the path + 1) x dir_words words
    long long layer_stride;
    const int* fpoff; const int* fprow; const int* fpslot;   // rows of every path, forward order
    const int* rpoff; const int* rprow; const int* rpslot;   // rows of every path, reverse order
    int nwv;                   // column stripes per read (see SweepArgs)
    int only_full;             // 1: only the reads k_trace flagged ST_LAYER_FULL (the fallback behind the windowed kernels, layer_window/)
};

// What the three layer kernels (k_layer, k_layer16, k_layer_win) settle for a read before their row loop: which path and which of
// its row lists (forward / reverse program order), the read and its (mirrored) columns, and the cell the traceback starts from —
// forward (fen | end row, rec_col | n), reverse (rsn, mirrored rec_col).  open() is false where there is nothing to rebuild: a read
// with one of the `skip` status bits (ST_RETRY: it is aligned again and its direction words may not exist), a reverse layer without a
// recombination, and — `heed_only_full`, the fallback launches behind the windowed kernel — a read k_trace did not flag.
struct LayerJob {
    ReadState* rs;
    int path;
    bool recomb;
    int n, ncols;
    const uint8_t* read;       // read[1 .. n]
    const int* prow; const int* pslot;
    int pbase, nrows;
    int start_row, start_col;
    int nx_row, nx_slot;       // look-ahead, stage one: the list entries of the next row to be fetched (-1: none)
    __device__ __forceinline__ bool open(const LayerArgs& a, int rd, uint32_t skip, bool heed_only_full) {
        rs = a.state + rd;
        if (rs->status & skip) return false;
        if (heed_only_full && a.only_full && !(rs->status & ST_LAYER_FULL)) return false;
        const bool rev = a.rev;
        path = rev ? rs->rev_path : rs->fwd_path;
        recomb = rs->fwd_path != rs->rev_path;
        if (rev && !recomb) return false;
        const long long ro = a.read_off[rd];
        n = (int)(a.read_off[rd + 1] - ro);
        read = a.reads + ro - 1;
        ncols = rev ? n : n + 1;
        prow = rev ? a.rprow : a.fprow;
        pslot = rev ? a.rpslot : a.fpslot;
        const int* poff = rev ? a.rpoff : a.fpoff;
        pbase = poff[path];
        nrows = poff[path + 1] - pbase;
        start_row = rev ? rs->rsn : (recomb ? rs->fen : rs->end_row);
        start_col = rev ? n - rs->rec_col : (recomb ? rs->rec_col : n);
        nx_row = -1; nx_slot = 0;
        return true;
    }
    // TWO-STAGE look-ahead.  A row needs its base code and its direction word, and their addresses come from the path's row / slot
    // lists: two DEPENDENT loads.  The list entries of row tt (of the first `upto` rows) are loaded here, while an earlier row is
    // computed; the loads they address are issued by the kernel one iteration later, when they have landed.
    __device__ __forceinline__ void fetch_idx(int tt, int upto) {
        nx_row = -1; nx_slot = 0;
        if (tt < upto) { nx_row = prow[pbase + tt]; nx_slot = pslot[pbase + tt]; }
    }
};

struct TraceArgs {
    PathGraphDev g;
    DevScores sc;
    const uint8_t* reads;
    const long long* read_off;
    ReadState* state;
    DevRecord* rec;
    uint8_t* ops;
    long long ops_stride;
    const int* flayer;
    const int* rlayer;
    long long layer_stride;
    const int* fpoff; const int* fprow;
    const int* rpoff; const int* rprow;
    int nreads;
    int mode;
    int semi;
    int nwv;                   // column stripes per read (see SweepArgs)
    // the layers were rebuilt inside a column window of `window` columns (layer_window/rg_layer_window.hpp; 0: full rows, today's
    // walk bit for bit): a walk that leaves the window or meets decision code 0 is abandoned, the read flagged ST_LAYER_FULL and
    // counted in *nfull.  only_full: walk the flagged reads only (their layers rebuilt at full width since) and clear the flag
    int window;
    int only_full;
    unsigned* nfull;
};

const char* launch_sweep(const SweepArgs& a, int nreads, int C, hipStream_t s);
const char* launch_sweep16(const SweepArgs& a, int nreads, int C, hipStream_t s);   // packed 16-bit rows (rg_sweep16.hip)
const char* launch_expand(const ExpandArgs& a, int nreads, int C, hipStream_t s);
const char* launch_colmax_rec(const ExpandArgs& a, int* colmax_out, int* colarg_out, int nreads, int C, hipStream_t s);
const char* launch_seed(const SeedArgs& a, hipStream_t s);
const char* launch_opt0(const Opt0Args& a, int nreads, int C, hipStream_t s);
const char* launch_opt0_16(const Opt0Args& a, int nreads, int C, hipStream_t s);   // packed rows (rg_sweep16.hip): batches the packed sweep admits
const char* launch_pick(const PickArgs& a, int nreads, hipStream_t s);
// Launch order of the sweeps' waves under path retirement: the work of a read grows with the highest id among its picked
// paths (every lower path leads it somewhere), from a few percent of a full sweep to all of it — longest first,
// so that the launch does not end on a few full-length waves (one block: counting sort by that id, descending).
const char* launch_order(const int* pick, const int* pick2, int* order, int nreads, hipStream_t s);
const char* launch_verify4(ReadState* st, const int* lb, unsigned* nretry, uint8_t* flags, int nreads, const int* dsel_pick, hipStream_t s);
const char* launch_verify(ReadState* st, const int* lb, unsigned* nretry, uint8_t* flags, int nreads, const int* dsel_pick, const int* dsel_pick2, int dsel_lo, int dsel_hi, hipStream_t s);
const char* launch_gather_reads(const uint8_t* reads, const long long* off, const int* idx, const long long* sub_off, uint8_t* out, int n, hipStream_t s);
const char* launch_scatter_results(const int* idx, const DevRecord* sub_rec, const uint8_t* sub_ops, DevRecord* rec, uint8_t* ops, long long ops_stride, int n, hipStream_t s);
const char* launch_threshold(const ThrArgs& a, int nreads, hipStream_t s);
const char* launch_bound(const BoundArgs& a, int nreads, hipStream_t s);
const char* launch_search(const SearchArgs& a, int nreads, hipStream_t s);
const char* launch_need(const ReadState* st, const unsigned* nf, const unsigned* nr, const unsigned* nrec, const unsigned* nrrec,
                 unsigned* need, int nreads, hipStream_t s);
const char* launch_layer(const LayerArgs& a, int nreads, int C, hipStream_t s);
const char* launch_layer16(const LayerArgs& a, int nreads, int C, hipStream_t s);   // packed rows (dir_fmt 1, one wave per read)
const char* launch_trace(const TraceArgs& a, int C, hipStream_t s);
// packed rows at C <= 16 inside a column window of `window` (128 | 256) columns around the walk (layer_window/rg_layer_window.hip)
const char* launch_layer_window(const LayerArgs& a, int nreads, int C, int window, hipStream_t s);

}  // namespace rg
