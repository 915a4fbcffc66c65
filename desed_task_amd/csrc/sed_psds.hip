// Threshold-free PSDS on the device: the per-(clip, class) step functions of desed_task_amd/evaluation/psds_scores.py::_clip_class_steps
// (the role of sed_scores_eval.intersection_based.psds, a third-party package: there is no reference call site).
//
// Per clip and class the detections as a function of the decision threshold are piecewise constant with break points at the
// clip's own <= T distinct scores, so the true-positive, false-positive and cross-trigger counts are step functions with at
// most T + 1 rows: row 0 = threshold below every score (all frames active), row i + 1 = threshold u[i].  One workgroup owns one
// (clip, class): it sorts the score column in LDS (bitonic, padded with +inf), compacts it to the distinct values, and then ONE
// THREAD PER THRESHOLD ROW walks the T frames -- all rows in lockstep, so the LDS reads of the score are broadcasts.  A run of
// active frames [a, b) is the detection [ts[a], ts[b]); its overlap with a ground-truth event is taken in closed form,
//     max(0, min(ts[b], off) - max(ts[a], on)),
// in float64 like the host: a run that touches no event yields exactly 0, which is what the `> 0` tests need.  The first walk
// classifies every run (relevant / false positive / cross trigger per other class) and leaves one relevance bit per run start in
// LDS; a second walk per ground-truth event of the class sums the event's coverage by the relevant runs.  Row counts go to LDS
// and their differences (the integer jumps between consecutive rows) are written out.  No atomics: two launches write
// identical bytes.
//
// Nothing here is multiplied and then added: the products (dtc * dur, gtc * dur_gt, cttc * dur) are only compared, so no
// contraction into an FMA can change a result.
#include "sed_common.h"
#include "../../include/sed_hip.h"   // SED_PSDS_MAX_T / SED_PSDS_MAX_NC: the limits the host shares

#define PSDS_THREADS 256
#define PSDS_T SED_PSDS_MAX_T
#define PSDS_NC SED_PSDS_MAX_NC
static_assert(PSDS_T == PSDS_THREADS, "one thread per threshold row and per sorted element");
// Row pitches of the per-row LDS tables, in dwords.  Each thread owns a row, so lane l touches row l: an odd pitch puts the 32 lanes
// of an access group on 32 different banks.
#define PSDS_REL_PITCH (PSDS_T / 32 + 1)
#define PSDS_CT_PITCH (PSDS_NC + 1)

struct PsdsArgs {
    const float* scores;       // (N, T, NC)
    const double* ts;          // (T + 1)
    const int* ev_ptr;         // (N * NC + 1)
    const double* ev_on;
    const double* ev_off;
    const double* clip_dur;    // (N)
    int* n_u;                  // (N * NC)
    float* u;                  // (N * NC, T)
    int* tp0;                  // (N * NC)
    int* fp0;                  // (N * NC)
    int* ct0;                  // (N * NC, NC)      count_ct only
    int* dtp;                  // (N * NC, T)
    int* dfp;                  // (N * NC, T)
    int* dct;                  // (N * NC, T, NC)   count_ct only
    double dtc, gtc, cttc;
    int T, NC, cttc_none, count_ct;
};

// summed overlap of [ta, tb) with the events e0 .. e1 - 1
__device__ __forceinline__ double psds_overlap(const double* __restrict__ on, const double* __restrict__ off, int e0, int e1,
                                               double ta, double tb) {
    double sum = 0.0;
    for (int e = e0; e < e1; ++e) {
        const double lo = fmax(ta, on[e]), hi = fmin(tb, off[e]);
        const double d = hi - lo;
        sum += d > 0.0 ? d : 0.0;
    }
    return sum;
}

__global__ __launch_bounds__(PSDS_THREADS) void psds_steps_kernel(const PsdsArgs p) {
    __shared__ double ts_l[PSDS_T + 1];
    __shared__ float s_l[PSDS_T];              // the score column, frame order
    __shared__ float srt[PSDS_T];              // sorted, then the distinct values
    __shared__ float u_l[PSDS_T];
    __shared__ int scan[2][PSDS_T];
    __shared__ int tp_l[PSDS_T + 1], fp_l[PSDS_T + 1];
    __shared__ unsigned rel_l[PSDS_T * PSDS_REL_PITCH];      // [row][word]: bit a = the run that starts at frame a is relevant
    __shared__ int ct_l[PSDS_T * PSDS_CT_PITCH];             // [row][class]
    __shared__ int n_u_l;

    const int T = p.T, NC = p.NC, tid = threadIdx.x;
    const int pair = blockIdx.x, clip = pair / NC, cls = pair - clip * NC;

    // ---- stage: frame boundaries, the score column, the sort buffer ------------------------------------------------------------
    for (int i = tid; i <= T; i += PSDS_THREADS) ts_l[i] = p.ts[i];
    {
        const float v = tid < T ? p.scores[((size_t)clip * T + tid) * NC + cls] : INFINITY;
        s_l[tid] = v;
        srt[tid] = v;
        u_l[tid] = INFINITY;
        tp_l[tid] = 0; fp_l[tid] = 0;
        if (tid == 0) { tp_l[PSDS_T] = 0; fp_l[PSDS_T] = 0; }
#pragma unroll
        for (int w = 0; w < PSDS_T / 32; ++w) rel_l[tid * PSDS_REL_PITCH + w] = 0u;
        if (p.count_ct)
            for (int k = 0; k < NC; ++k) ct_l[tid * PSDS_CT_PITCH + k] = 0;
    }
    __syncthreads();

    // ---- bitonic sort of the 256 padded values, ascending -------------------------------------------------------------------------
    for (int k = 2; k <= PSDS_T; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int other = tid ^ j;
            if (other > tid) {
                const float a = srt[tid], b = srt[other];
                const bool asc = (tid & k) == 0;
                if ((a > b) == asc && a != b) { srt[tid] = b; srt[other] = a; }
            }
            __syncthreads();
        }
    }

    // ---- compact to the distinct values: inclusive scan of "first of its value" ---------------------------------------------------
    const float mine = srt[tid];
    const int first = (tid < T && (tid == 0 || mine != srt[tid - 1])) ? 1 : 0;
    scan[0][tid] = first;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < PSDS_T; d <<= 1) {
        const int v = scan[cur][tid] + (tid >= d ? scan[cur][tid - d] : 0);
        scan[cur ^ 1][tid] = v;
        cur ^= 1;
        __syncthreads();
    }
    if (first) u_l[scan[cur][tid] - 1] = mine;
    if (tid == PSDS_T - 1) n_u_l = scan[cur][tid];
    __syncthreads();
    const int n_u = n_u_l;

    // ---- one thread per threshold row ------------------------------------------------------------------------------------------------
    const int* __restrict__ ev_ptr = p.ev_ptr + (size_t)clip * NC;       // this clip's classes: events of class k are ev_ptr[k] .. ev_ptr[k + 1] - 1
    const double* __restrict__ ev_on = p.ev_on;
    const double* __restrict__ ev_off = p.ev_off;
    const int g0 = ev_ptr[cls], g1 = ev_ptr[cls + 1];
    const bool row_live = tid < n_u;                                      // row n_u (threshold = the largest score) detects nothing
    const float thr = tid == 0 ? -INFINITY : u_l[tid > 0 ? tid - 1 : 0];
    const double clip_dur = p.clip_dur[clip];

    if (row_live) {
        int fp = 0, a = -1;
        for (int t = 0; t <= T; ++t) {
            const bool active = t < T && s_l[t] > thr;
            if (active) {
                if (a < 0) a = t;
            } else if (a >= 0) {
                const double ta = ts_l[a], tb = ts_l[t], dur = tb - ta;
                const double same = psds_overlap(ev_on, ev_off, g0, g1, ta, tb);
                if (same > 0.0 && same >= p.dtc * dur) {
                    rel_l[tid * PSDS_REL_PITCH + (a >> 5)] |= 1u << (a & 31);
                } else {
                    const double hi = fmin(tb, clip_dur), lo = fmax(ta, 0.0), wd = hi - lo;
                    const double w = wd > 0.0 ? wd : 0.0;
                    if (w > 0.0 && (p.cttc_none || w >= p.cttc * dur)) ++fp;
                    if (p.count_ct) {
                        for (int k = 0; k < NC; ++k) {
                            if (k == cls) continue;
                            const int e0 = ev_ptr[k], e1 = ev_ptr[k + 1];
                            if (e0 == e1) continue;
                            const double x = psds_overlap(ev_on, ev_off, e0, e1, ta, tb);
                            if (x > 0.0 && x >= p.cttc * dur) ct_l[tid * PSDS_CT_PITCH + k] += 1;
                        }
                    }
                }
                a = -1;
            }
        }
        fp_l[tid] = fp;

        // coverage of every ground-truth event of the class by the relevant runs of this row
        int tp = 0;
        for (int g = g0; g < g1; ++g) {
            const double on = ev_on[g], off = ev_off[g];
            double cover = 0.0;
            a = -1;
            for (int t = 0; t <= T; ++t) {
                const bool active = t < T && s_l[t] > thr;
                if (active) {
                    if (a < 0) a = t;
                } else if (a >= 0) {
                    if ((rel_l[tid * PSDS_REL_PITCH + (a >> 5)] >> (a & 31)) & 1u) {
                        const double lo = fmax(ts_l[a], on), hi = fmin(ts_l[t], off), d = hi - lo;
                        cover += d > 0.0 ? d : 0.0;
                    }
                    a = -1;
                }
            }
            if (cover >= p.gtc * (off - on)) ++tp;
        }
        tp_l[tid] = tp;
    }
    __syncthreads();

    // ---- write: distinct scores, row 0, jumps between consecutive rows ---------------------------------------------------------------
    const size_t po = (size_t)pair;
    if (tid == 0) {
        p.n_u[po] = n_u;
        p.tp0[po] = tp_l[0];
        p.fp0[po] = fp_l[0];
    }
    if (tid < T) {
        p.u[po * T + tid] = u_l[tid];
        const bool live = tid < n_u;                                       // jump i: row i -> row i + 1 (row n_u holds zeros)
        p.dtp[po * T + tid] = live ? tp_l[tid + 1] - tp_l[tid] : 0;
        p.dfp[po * T + tid] = live ? fp_l[tid + 1] - fp_l[tid] : 0;
    }
    if (p.count_ct) {
        if (tid < NC) p.ct0[po * NC + tid] = ct_l[tid];
        int* __restrict__ out = p.dct + po * T * NC;
        for (int i = tid; i < T * NC; i += PSDS_THREADS) {
            const int row = i / NC, k = i - row * NC;
            int v = 0;
            if (row < n_u) v = (row + 1 < n_u ? ct_l[(row + 1) * PSDS_CT_PITCH + k] : 0) - ct_l[row * PSDS_CT_PITCH + k];
            out[i] = v;
        }
    }
}

SED_API int sed_psds_steps(const float* scores, const double* ts, const int* ev_ptr, const double* ev_on, const double* ev_off,
                           const double* clip_dur, int N, int T, int NC, double dtc, double gtc, double cttc, int cttc_none,
                           int count_ct, int* n_u, float* u, int* tp0, int* fp0, int* ct0, int* dtp, int* dfp, int* dct,
                           void* stream) {
    if (N <= 0) return SED_OK;
    if (T < 1 || NC < 1) return SED_ERR_ARG;
    if (T > SED_PSDS_MAX_T || NC > SED_PSDS_MAX_NC) return SED_ERR_UNSUPPORTED;
    if ((long long)N * NC >= (1ll << 31)) return SED_ERR_UNSUPPORTED;
    if (!scores || !ts || !ev_ptr || !clip_dur || !n_u || !u || !tp0 || !fp0 || !dtp || !dfp) return SED_ERR_ARG;
    if (count_ct && (cttc_none || !ct0 || !dct)) return SED_ERR_ARG;
    PsdsArgs p;
    p.scores = scores; p.ts = ts; p.ev_ptr = ev_ptr; p.ev_on = ev_on; p.ev_off = ev_off; p.clip_dur = clip_dur;
    p.n_u = n_u; p.u = u; p.tp0 = tp0; p.fp0 = fp0; p.ct0 = ct0; p.dtp = dtp; p.dfp = dfp; p.dct = dct;
    p.dtc = dtc; p.gtc = gtc; p.cttc = cttc;
    p.T = T; p.NC = NC; p.cttc_none = cttc_none ? 1 : 0; p.count_ct = count_ct ? 1 : 0;
    SED_LAUNCH(psds_steps_kernel, dim3((unsigned)(N * NC)), dim3(PSDS_THREADS), 0, (hipStream_t)stream, p);
    return sed_check_launch();
}
