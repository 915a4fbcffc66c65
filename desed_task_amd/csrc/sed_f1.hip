// Collar, segment and intersection F1 counts on the device: what evaluation_measures.log_sedeval_metrics (sed_eval's event-based and
// segment-based metrics, evaluation/sed_eval_metrics.py) and compute_per_intersection_macro_f1 (psds_eval's F score,
// evaluation/psds.py::_evaluate_detections) count per (threshold, clip, class), as eight integers.  Third-party roles: there is no
// reference call site below desed_task/evaluation/evaluation_measures.py:50-195.
//
// One single-wave workgroup owns one clip and up to 64 of its n_thr * NC (threshold, class) columns; a lane owns one column.  The
// clip's (T, NC) score tile is staged in (dynamic, shape-sized) LDS once with coalesced reads (row pitch NC | 1).  The lane walks its column -- all lanes
// at the same frame, so lanes of one class at different thresholds read one LDS word (a broadcast) and lanes of different classes
// hit different banks -- and leaves its runs of `score > thr` (strict, fp32, as threshold_events_kernel) in LDS as 16-bit words
// (a | (b - 1) << 8 for the run [a, b), T <= 256; layout [run][lane], so the lanes of an access touch consecutive half words).  A run
// is the event [ts[a], ts[b]): ts is an input and is never recomputed.  The per-event passes then read the run list:
//
//   collar_tp   maximum bipartite matching under EventBasedMetrics._time_match.  The runs of a column are disjoint and ascending in
//               onset AND offset, so the runs an event may match are a contiguous index range [lo, hi] (two interval conditions
//               intersected), also when the events of the class overlap each other.  On such a convex graph "walk the runs in order
//               and give each to the open, unmatched event with the smallest hi" is a maximum matching (Glover's rule): no
//               recursion, no augmenting paths.  lo / hi per event sit in LDS as bytes.
//   seg_*       64-bit rasters [floor(on / res), ceil(off / res)) of the events and of the runs, and popcounts.
//   int_tp/fp   psds.py's arithmetic form: a RATIO per (run, event) pair, inter / dur_run or inter / dur_gt, then a sum in
//               ground-truth order resp. run order (np.bincount's order), compared with dtc / gtc / cttc.  (sed_psds.hip compares a
//               summed overlap with dtc * dur instead: a different rounding, on purpose not shared.)  Relevance bits of the <= 128
//               runs live in two 64-bit registers.
//
// All time arithmetic is float64.  Nothing here is a multiply followed by an add -- the one product, percentage_of_length * (off -
// on), only enters a max and a comparison, and the sums add quotients -- so hipcc's default contraction into FMAs cannot move a
// comparison.  Keep it that way.  Plain stores, no atomics: two launches write identical bytes.  Cross-trigger counts are not
// needed for an F score and are not computed.
#include "sed_common.h"
#include "../../include/sed_hip.h"   // SED_F1_*: the limits the host shares

#define F1_THREADS 64
#define F1_T SED_F1_MAX_T
#define F1_NC SED_F1_MAX_NC
#define F1_RUNS ((F1_T + 1) / 2)
#define F1_EV SED_F1_MAX_EVENTS
static_assert(F1_T <= 256, "a run [a, b) is packed as a | (b - 1) << 8");
static_assert(F1_RUNS <= 128, "relevance bits of a column's runs: two 64-bit registers");
static_assert(F1_RUNS <= 255, "lo / hi of an event's run range are bytes, 255 = no run");
static_assert(F1_EV <= 32, "matched events of a column: one 32-bit register");
static_assert(SED_F1_MAX_CELLS == 64, "a raster is one 64-bit register");

struct F1Args {
    const float* scores;       // (N, T, NC)
    const float* thr;          // (n_thr)
    const double* ts;          // (T + 1)
    const int* ev_ptr;         // (N * NC + 1)
    const double* ev_on;
    const double* ev_off;
    const double* clip_dur;    // (N)
    int* counts;               // (n_thr, N, NC, 8)
    double t_collar, pct, res, dtc, gtc, cttc;
    int N, T, NC, n_thr, groups;
};

// bits [lo, hi) of a 64-cell raster, from the cell bounds as doubles
__device__ __forceinline__ unsigned long long f1_cells(double on_cell, double off_cell) {
    const int lo = (int)fmin(fmax(on_cell, 0.0), 64.0), hi = (int)fmin(fmax(off_cell, 0.0), 64.0);
    if (hi <= lo) return 0ull;
    const unsigned long long upto_hi = hi >= 64 ? ~0ull : (1ull << hi) - 1ull;
    return upto_hi & ~((1ull << lo) - 1ull);                      // lo < hi <= 64: lo <= 63
}

__global__ __launch_bounds__(F1_THREADS) void f1_counts_kernel(const F1Args p) {
    // dynamic LDS sized by the shape (the recipe's 156 x 10 clip takes 22 KB, the limits 55 KB): ts, tile, runs, lo, hi
    SED_DYN_SMEM(smem);
    const int T = p.T, NC = p.NC, N = p.N, tid = threadIdx.x;
    const int clip = blockIdx.x / p.groups, group = blockIdx.x - clip * p.groups;
    const int pitch = NC | 1, max_runs = (T + 1) / 2;
    double* ts_l = (double*)smem;                                                     // [T + 1]
    float* tile = (float*)(ts_l + T + 1);                                             // [frame][class], pitch NC | 1
    unsigned short* run_l = (unsigned short*)(tile + T * pitch);                      // [run][lane]
    unsigned char* lo_l = (unsigned char*)(run_l + max_runs * F1_THREADS);            // [event][lane]
    unsigned char* hi_l = lo_l + F1_EV * F1_THREADS;

    // ---- stage the clip's tile and the frame boundaries ------------------------------------------------------------------------------
    const float* __restrict__ src = p.scores + (size_t)clip * T * NC;
    for (int i = tid; i < T * NC; i += F1_THREADS) {
        const int t = i / NC, c = i - t * NC;
        tile[t * pitch + c] = src[i];
    }
    for (int i = tid; i <= T; i += F1_THREADS) ts_l[i] = p.ts[i];
    __syncthreads();

    const int col = group * F1_THREADS + tid;
    if (col >= p.n_thr * NC) return;
    const int k = col / NC, cls = col - k * NC;
    const float thr = p.thr[k];

    // ---- walk: the runs of score > thr -----------------------------------------------------------------------------------------------
    int n_runs = 0;
    {
        int a = -1;
        for (int t = 0; t <= T; ++t) {
            const bool active = t < T && tile[t * pitch + cls] > thr;
            if (active) {
                if (a < 0) a = t;
            } else if (a >= 0) {
                run_l[n_runs * F1_THREADS + tid] = (unsigned short)(a | ((t - 1) << 8));      // n_runs < (T + 1) / 2 by construction
                ++n_runs;
                a = -1;
            }
        }
    }
#define F1_RUN(r, on_s, off_s) \
    const unsigned rw_ = run_l[(r) * F1_THREADS + tid]; \
    const double on_s = ts_l[rw_ & 255u], off_s = ts_l[(rw_ >> 8) + 1u]

    const double* __restrict__ ev_on = p.ev_on;
    const double* __restrict__ ev_off = p.ev_off;
    const int g0 = p.ev_ptr[(size_t)clip * NC + cls];
    int g1 = p.ev_ptr[(size_t)clip * NC + cls + 1];
    if (g1 - g0 > F1_EV) g1 = g0 + F1_EV;                          // the host layer refuses such a table before any launch
    const int n_ev = g1 - g0;

    // ---- collar: the run range of every event, then the greedy matching -------------------------------------------------------------
    int collar_tp = 0;
    if (n_ev > 0 && n_runs > 0) {
        for (int e = 0; e < n_ev; ++e) {
            const double on_r = ev_on[g0 + e], off_r = ev_off[g0 + e];
            const double tol = fmax(p.t_collar, p.pct * (off_r - on_r));
            int lo = 255, hi = 0;
            for (int r = 0; r < n_runs; ++r) {
                F1_RUN(r, on_s, off_s);
                if (on_s - on_r > p.t_collar) break;              // onsets ascend: no later run can match either
                if (fabs(on_r - on_s) <= p.t_collar && fabs(off_r - off_s) <= tol) {
                    if (lo == 255) lo = r;
                    hi = r;
                }
            }
            lo_l[e * F1_THREADS + tid] = (unsigned char)lo;
            hi_l[e * F1_THREADS + tid] = (unsigned char)hi;
        }
        unsigned matched = 0u;
        for (int r = 0; r < n_runs; ++r) {
            int best = -1, best_hi = 256;
            for (int e = 0; e < n_ev; ++e) {
                if ((matched >> e) & 1u) continue;
                const int lo = lo_l[e * F1_THREADS + tid], hi = hi_l[e * F1_THREADS + tid];
                if (lo <= r && r <= hi && hi < best_hi) { best = e; best_hi = hi; }
            }
            if (best >= 0) { matched |= 1u << best; ++collar_tp; }
        }
    }

    // ---- segments: 64-cell rasters ---------------------------------------------------------------------------------------------------
    unsigned long long ref_cells = 0ull, sys_cells = 0ull;
    for (int e = g0; e < g1; ++e) ref_cells |= f1_cells(floor(ev_on[e] / p.res), ceil(ev_off[e] / p.res));
    for (int r = 0; r < n_runs; ++r) {
        F1_RUN(r, on_s, off_s);
        sys_cells |= f1_cells(floor(on_s / p.res), ceil(off_s / p.res));
    }

    // ---- intersection: relevant runs and false positives, then the events they hit --------------------------------------------------
    const double clip_dur = p.clip_dur[clip];
    unsigned long long rel0 = 0ull, rel1 = 0ull;
    int int_fp = 0, int_tp = 0;
    for (int r = 0; r < n_runs; ++r) {
        F1_RUN(r, on_s, off_s);
        const double dur = off_s - on_s;
        double sum = 0.0;
        bool has = false;
        for (int e = g0; e < g1; ++e) {
            const double inter = fmin(off_s, ev_off[e]) - fmax(on_s, ev_on[e]);
            if (inter > 0.0) { sum += inter / dur; has = true; }
        }
        if (has && sum >= p.dtc) {
            if (r < 64) rel0 |= 1ull << r; else rel1 |= 1ull << (r - 64);
        } else {
            const double w = fmin(off_s, clip_dur) - fmax(on_s, 0.0);
            if (w > 0.0 && w / dur >= p.cttc) ++int_fp;
        }
    }
    if (rel0 | rel1) {
        for (int e = g0; e < g1; ++e) {
            const double on_r = ev_on[e], off_r = ev_off[e], dur_gt = off_r - on_r;
            double sum = 0.0;
            bool has = false;
            for (int r = 0; r < n_runs; ++r) {
                if (!(((r < 64 ? rel0 >> r : rel1 >> (r - 64))) & 1ull)) continue;
                F1_RUN(r, on_s, off_s);
                const double inter = fmin(off_s, off_r) - fmax(on_s, on_r);
                if (inter > 0.0) { sum += inter / dur_gt; has = true; }
            }
            if (has && sum >= p.gtc) ++int_tp;
        }
    }
#undef F1_RUN

    int4* __restrict__ out = (int4*)(p.counts + (((size_t)k * N + clip) * NC + cls) * 8);
    out[0] = make_int4(n_runs, collar_tp, __builtin_popcountll(ref_cells), __builtin_popcountll(sys_cells));
    out[1] = make_int4(__builtin_popcountll(ref_cells & sys_cells), int_tp, int_fp, 0);
}

SED_API int sed_f1_counts(const float* scores, const float* thr, const double* ts, const int* ev_ptr, const double* ev_on,
                          const double* ev_off, const double* clip_dur, int N, int T, int NC, int n_thr, double t_collar,
                          double percentage_of_length, double time_resolution, double dtc, double gtc, double cttc, int* counts,
                          void* stream) {
    if (N <= 0) return SED_OK;
    if (T < 1 || NC < 1 || n_thr < 1 || !(time_resolution > 0.0)) return SED_ERR_ARG;
    if (T > SED_F1_MAX_T || NC > SED_F1_MAX_NC || n_thr > SED_F1_MAX_THR) return SED_ERR_UNSUPPORTED;
    const int groups = (n_thr * NC + F1_THREADS - 1) / F1_THREADS;
    if ((long long)N * NC * n_thr * 8 >= (1ll << 31) || (long long)N * groups >= (1ll << 31)) return SED_ERR_UNSUPPORTED;
    if (!scores || !thr || !ts || !ev_ptr || !clip_dur || !counts || ((uintptr_t)counts & 15u)) return SED_ERR_ARG;
    F1Args p;
    p.scores = scores; p.thr = thr; p.ts = ts; p.ev_ptr = ev_ptr; p.ev_on = ev_on; p.ev_off = ev_off; p.clip_dur = clip_dur;
    p.counts = counts;
    p.t_collar = t_collar; p.pct = percentage_of_length; p.res = time_resolution; p.dtc = dtc; p.gtc = gtc; p.cttc = cttc;
    p.N = N; p.T = T; p.NC = NC; p.n_thr = n_thr; p.groups = groups;
    const size_t smem = (size_t)(T + 1) * sizeof(double) + (size_t)T * (NC | 1) * sizeof(float)
                        + (size_t)((T + 1) / 2) * F1_THREADS * sizeof(unsigned short) + 2 * F1_EV * F1_THREADS;     // <= 56 328 bytes
    SED_LAUNCH(f1_counts_kernel, dim3((unsigned)(N * groups)), dim3(F1_THREADS), smem, (hipStream_t)stream, p);
    return sed_check_launch();
}
