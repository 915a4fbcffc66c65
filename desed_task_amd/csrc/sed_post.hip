// K13: inference post-processing of the frame-level posteriors on the device, replacing the per-clip
// `.cpu().numpy()` loop of recipes/dcase2023_task4_baseline/local/utils.py:16-73 (batched_decode_preds):
//   * sed_median_filter    : scipy.ndimage.median_filter(scores (T, NC), size=(win, 1)) for every clip of the batch --
//                            median over time with scipy's default 'reflect' boundary (d c b a | a b c d | d c b a),
//                            window centred with origin 0 (covers t - win/2 .. t + (win-1)/2); utils.py:55;
//   * sed_threshold_events : `scores > threshold` (utils.py:62) followed by the contiguous-region search that
//                            ManyHotEncoder.decode_strong (desed_task/utils/encoder.py:189-211) delegates to
//                            dcase_util's DecisionEncoder.find_contiguous_regions: [onset_frame, offset_frame) pairs per
//                            (threshold, clip, class), in frame units; the host only converts frames to seconds.
//   * sed_median_filter_classwise : the 2024 recipe's ClassWiseMedianFilter (desed_task/utils/postprocess.py:5-18, called from
//                            recipes/dcase2024_task4_baseline/local/utils.py:77 through sed_trainer_pretrained.py:545,561,872,896):
//                            scipy.ndimage.median_filter(x[:, c:c+1], (wins[c], 1)) per class c, one window length per class;
//   * sed_segment_scores   : 10 s clip frame scores -> 1 s segment scores of the 2024 test path, mode 0 = the overlap-weighted
//                            mean of _get_segment_scores (recipes/dcase2024_task4_baseline/local/sed_trainer_pretrained.py:1457-1490),
//                            mode 1 = the segment maximum that the segment-based evaluator (evaluation/segment_based.py) scores.
// Layout: scores (B, T, NC) frame-major, the native layout of the head kernel (the reference's (B, NC, T) tensor is a
// transposed view of it).  Integer / selection work: results are bit-exact.
#include "sed_common.h"

#define POST_MAX_WIN 15

// index of the reflected sample: period 2T, ... 2 1 0 | 0 1 2 ... T-1 | T-1 T-2 ...
__device__ __forceinline__ int reflect_index(int i, int T) {
    const int p = 2 * T;
    i %= p;
    if (i < 0) i += p;
    return i < T ? i : p - 1 - i;
}

__global__ __launch_bounds__(256) void median_filter_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int T,
                                                            int NC, int win) {
    const size_t n = (size_t)B * T * NC;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const int c = (int)(e % NC), t = (int)((e / NC) % T);
        const size_t b = e / ((size_t)NC * T);
        const float* col = x + b * T * NC + c;
        float v[POST_MAX_WIN];
#pragma unroll
        for (int k = 0; k < POST_MAX_WIN; ++k)
            if (k < win) v[k] = col[(size_t)reflect_index(t - win / 2 + k, T) * NC];
        // insertion sort of <= 15 values (fully unrolled: the array stays in registers); NaNs are not expected in posteriors
#pragma unroll
        for (int a = 1; a < POST_MAX_WIN; ++a) {
            if (a < win) {
#pragma unroll
                for (int b2 = POST_MAX_WIN - 1; b2 >= 1; --b2) {
                    if (b2 <= a) {
                        const float lo = fminf(v[b2 - 1], v[b2]), hi = fmaxf(v[b2 - 1], v[b2]);
                        v[b2 - 1] = lo; v[b2] = hi;
                    }
                }
            }
        }
        float m = v[0];
#pragma unroll
        for (int k = 0; k < POST_MAX_WIN; ++k)
            if (k == win / 2) m = v[k];
        y[e] = m;
    }
}

// scores (B,T,NC) -> out (B,T,NC); win odd or even, 1 <= win <= 15 (scipy picks element win/2 of the sorted window).
SED_API int sed_median_filter(const float* scores, float* out, int B, int T, int NC, int win, void* stream) {
    if (win < 1 || win > POST_MAX_WIN) return SED_ERR_UNSUPPORTED;
    if (B <= 0 || T <= 0 || NC <= 0) return SED_OK;
    const size_t n = (size_t)B * T * NC;
    int grid = (int)((n + 255) / 256);
    if (grid > 4096) grid = 4096;
    SED_LAUNCH(median_filter_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, scores, out, B, T, NC, win);
    return sed_check_launch();
}

// One thread per (threshold, clip, class): walks the frames once and appends [onset, offset) pairs.
// counts (n_thr, B, NC) int32; events (n_thr, B, NC, max_events, 2) int32.  true_len (B) int32 or null: frames past it are
// ignored (utils.py:48-50, padded clips).  A (clip, class) column cannot hold more than (T + 1) / 2 regions.
__global__ __launch_bounds__(256) void threshold_events_kernel(const float* __restrict__ scores, const float* __restrict__ thr,
                                                               const int* __restrict__ true_len, int* __restrict__ counts,
                                                               int* __restrict__ events, int B, int T, int NC, int n_thr,
                                                               int max_events) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_thr * B * NC) return;
    const int c = idx % NC, b = (idx / NC) % B, k = idx / (NC * B);
    const float th = thr[k];
    const int len = true_len ? min(max(true_len[b], 0), T) : T;
    const float* col = scores + (size_t)b * T * NC + c;
    int* ev = events + (size_t)idx * max_events * 2;
    int n = 0, onset = -1;
    for (int t = 0; t < len; ++t) {
        const bool on = col[(size_t)t * NC] > th;
        if (on && onset < 0) onset = t;
        if (!on && onset >= 0) {
            if (n < max_events) { ev[2 * n] = onset; ev[2 * n + 1] = t; }
            ++n; onset = -1;
        }
    }
    if (onset >= 0) {
        if (n < max_events) { ev[2 * n] = onset; ev[2 * n + 1] = len; }
        ++n;
    }
    counts[idx] = n;
}

SED_API int sed_threshold_events(const float* scores, const float* thresholds, const int* true_len, int* counts, int* events,
                                    int B, int T, int NC, int n_thr, int max_events, void* stream) {
    if (n_thr <= 0 || max_events < (T + 1) / 2) return SED_ERR_ARG;
    if (B <= 0 || T <= 0 || NC <= 0) return SED_OK;
    const int n = n_thr * B * NC;
    SED_LAUNCH(threshold_events_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, scores, thresholds, true_len, counts,
               events, B, T, NC, n_thr, max_events);
    return sed_check_launch();
}

// ---- class-wise median filter (2024 recipe) ------------------------------------------------------------------------------------
// One workgroup per (tile of CLS_TT output frames, block of CLS_CB classes, clip).  The tile's CLS_TT + w_max - 1 reflected input
// rows of those classes are staged in LDS once (coalesced along the class axis); every lane then takes its (frame, class) window
// out of LDS into registers -- N slots, the w real samples and +inf behind them -- and sorts them with a bitonic network whose
// indices are all compile-time constants (the array stays in VGPRs).  Element w/2 of the sorted slots is scipy's median (the +inf
// pads sort to the end).  N = 16 / 32 / 64 is the smallest tier >= w_max, chosen on the host.  Selection only: bit-exact.
#define CLS_MAX_WIN 64
#define CLS_TT 32
#define CLS_CB 32
#define CLS_LD 33   // LDS row pitch in floats: lanes of one class at different frames fall on different banks

template <int N>
__device__ __forceinline__ void bitonic_sort(float (&v)[N]) {
#pragma unroll
    for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const float lo = fminf(v[i], v[l]), hi = fmaxf(v[i], v[l]);
                    if ((i & k) == 0) { v[i] = lo; v[l] = hi; }
                    else              { v[i] = hi; v[l] = lo; }
                }
            }
        }
    }
}

template <int N>
__global__ __launch_bounds__(256) void median_classwise_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                               const int* __restrict__ wins, int T, int NC, int w_max) {
    __shared__ float s[(CLS_TT + CLS_MAX_WIN - 1) * CLS_LD];
    __shared__ int sw[CLS_CB];
    const int t0 = blockIdx.x * CLS_TT, c0 = blockIdx.y * CLS_CB, b = blockIdx.z;
    const int ncb = min(CLS_CB, NC - c0);
    const int half = w_max / 2, rows = CLS_TT + w_max - 1;
    const float* xb = x + (size_t)b * T * NC + c0;
    if ((int)threadIdx.x < ncb) sw[threadIdx.x] = min(max(wins[c0 + threadIdx.x], 1), w_max);
    // staged row r holds input frame t0 + r - w_max/2, reflected into [0, T) (any number of times when T < w_max)
    for (int i = threadIdx.x; i < rows * ncb; i += 256) {
        const int r = i / ncb, c = i - r * ncb;
        s[r * CLS_LD + c] = xb[(size_t)reflect_index(t0 + r - half, T) * NC + c];
    }
    __syncthreads();
    const int nt = min(CLS_TT, T - t0);
    for (int e = threadIdx.x; e < nt * ncb; e += 256) {
        const int t = e / ncb, c = e - t * ncb;
        const int w = sw[c];
        // window of frame t: frames t - w/2 .. t + (w-1)/2 = staged rows t + half - w/2 .. t + half - w/2 + w - 1 <= t + w_max - 1
        const float* col = s + (t + half - w / 2) * CLS_LD + c;
        float v[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const float a = col[min(k, w - 1) * CLS_LD];
            v[k] = k < w ? a : __builtin_inff();
        }
        bitonic_sort<N>(v);
        float m = v[0];
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k == w / 2) m = v[k];
        y[((size_t)b * T + t0 + t) * NC + c0 + c] = m;
    }
}

// scores (B,T,NC) -> out (B,T,NC); wins (NC) int32 on the device, each in [1, w_max]; w_max <= 64 (host-known: the largest entry).
// Contract: an entry outside [1, w_max] cannot be reported from the device; it is clamped into that range (every LDS read stays
// inside the staged rows) and its class is filtered with the clamped length.
SED_API int sed_median_filter_classwise(const float* scores, float* out, const int* wins, int B, int T, int NC, int w_max,
                                        void* stream) {
    if (w_max < 1 || w_max > CLS_MAX_WIN) return SED_ERR_UNSUPPORTED;
    if (B <= 0 || T <= 0 || NC <= 0) return SED_OK;
    if (B > 65535) return SED_ERR_ARG;
    const dim3 grid((T + CLS_TT - 1) / CLS_TT, (NC + CLS_CB - 1) / CLS_CB, B);
    hipStream_t s = (hipStream_t)stream;
    if (w_max <= 16)      SED_LAUNCH(median_classwise_kernel<16>, grid, dim3(256), 0, s, scores, out, wins, T, NC, w_max);
    else if (w_max <= 32) SED_LAUNCH(median_classwise_kernel<32>, grid, dim3(256), 0, s, scores, out, wins, T, NC, w_max);
    else                  SED_LAUNCH(median_classwise_kernel<64>, grid, dim3(256), 0, s, scores, out, wins, T, NC, w_max);
    return sed_check_launch();
}

// ---- frame scores -> segment scores (2024 test path) -----------------------------------------------------------------------------
// One thread per (clip, segment, class).  Frame i spans [i*hop, (i+1)*hop); segment k starts at k*L and exists while k <
// ceil(clip_len[b] / L) (np.arange(0, clip_len, L)); times and weights in double, as the reference's float64 timestamps.
//   mode 0 (_get_segment_scores, sed_trainer_pretrained.py:1457-1490): the frames with end > k*L and start < k*L + L (the segment
//          end is NOT clipped to the clip there, so the last, partial segment averages every frame that starts before k*L + L),
//          weights min(t_{i+1}, k*L + L) - max(t_i, k*L), score = sum(w * s) / sum(w);
//   mode 1: the maximum over the frames that overlap [k*L, min(k*L + L, clip_len)) with positive length, 0 when none does.
// Segments at or past the clip's own count are written as 0.
__global__ __launch_bounds__(256) void segment_scores_kernel(const float* __restrict__ x, const float* __restrict__ clip_len,
                                                             float* __restrict__ y, int B, int T, int NC, double hop, double L,
                                                             int n_seg, int mode) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)B * n_seg * NC) return;
    const int c = (int)(idx % NC), k = (int)((idx / NC) % n_seg), b = (int)(idx / ((long long)NC * n_seg));
    const double len = (double)clip_len[b];
    float r = 0.f;
    if (k < (int)ceil(len / L)) {
        const double on = k * L;
        const double off = mode == 0 ? on + L : fmin(on + L, len);
        const float* col = x + (size_t)b * T * NC + c;
        // only frames in [i_lo, i_hi) can overlap [on, off)
        const int i_lo = max(0, (int)floor(on / hop) - 1), i_hi = min(T, (int)ceil(off / hop) + 1);
        double num = 0.0, den = 0.0;
        float m = -__builtin_inff();
        bool any = false;
        for (int i = i_lo; i < i_hi; ++i) {
            const double ta = i * hop, tb = (i + 1) * hop;
            if (tb > on && ta < off) {
                const float v = col[(size_t)i * NC];
                const double w = fmin(tb, off) - fmax(ta, on);
                num += w * (double)v;
                den += w;
                m = fmaxf(m, v);
                any = true;
            }
        }
        r = mode == 0 ? (float)(num / den) : (any ? m : 0.f);
    }
    y[idx] = r;
}

// scores (B,T,NC), clip_len (B) float seconds on the device -> out (B,n_seg,NC).  mode 0 = weighted mean, 1 = maximum.
SED_API int sed_segment_scores(const float* scores, const float* clip_len, float* out, int B, int T, int NC, double frame_hop,
                               double seg_len, int n_seg, int mode, void* stream) {
    if ((mode != 0 && mode != 1) || !(frame_hop > 0.0) || !(seg_len > 0.0)) return SED_ERR_ARG;
    if (B <= 0 || T <= 0 || NC <= 0 || n_seg <= 0) return SED_OK;
    const long long n = (long long)B * n_seg * NC;
    SED_LAUNCH(segment_scores_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, scores, clip_len, out,
               B, T, NC, frame_hop, seg_len, n_seg, mode);
    return sed_check_launch();
}
