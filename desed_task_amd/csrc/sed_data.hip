// Resident training set: one launch assembles one batch from pools that live in HBM (desed_task_amd/resident.py).
// What it replaces is the reference's per-item host path -- torchaudio.load + label encoding in
// desed_task/dataio/datasets.py:60-74,187-237, default_collate and the DataLoader of local/sed_trainer.py:913-920, then a 30 MB
// host-to-device copy per step -- by, for every stream s (waveforms, labels, embeddings, class mask) and every output row b,
//     out_s[b, :] = convert_s(pool_s[idx[b], :]).
//
// HBM-bound: algorithmic bytes per row = len * (input + output element size); the B = 48 x 10 s batch of the 2023 recipe reads
// 15.4 MB of 16-bit samples and writes 30.7 MB of floats.  A workgroup owns SED_GATHER_CHUNK consecutive output elements of ONE row
// of ONE stream, so the grid follows the bytes (640 KB of waveform = 40 workgroups per row, a label matrix = 1), and everything
// that selects its work -- the stream, the row, the row's index -- is uniform: scalar loads, one index read per workgroup.
// Pool rows start on 16-byte boundaries (the pool's row stride is padded to a multiple of 16 bytes); output rows are dense (B, len),
// so a row whose start is not 16-byte aligned (odd len) is copied element-wise, every other row as 16-byte loads and stores plus an
// element-wise tail of len % (elements per 16 input bytes).  Plain stores: the step's first kernels read the batch right away.
//
// The kernel checks NO index: 0 <= idx[b] < rows of every pool is the host's contract (resident.py validates the whole epoch's
// table before it uploads it).
#include "sed_common.h"
#include "../../include/sed_hip.h"   // SED_GATHER_*: the descriptor layout, the kinds and the chunk the host shares

#define GATHER_THREADS 256
#define GATHER_CHUNK SED_GATHER_CHUNK       // output elements per workgroup
enum { GATHER_I16_TO_F32 = SED_GATHER_I16_TO_F32, GATHER_F32 = SED_GATHER_F32, GATHER_U8_TO_F32 = SED_GATHER_U8_TO_F32,
       GATHER_U8 = SED_GATHER_U8 };

// The pool and output pointers come out of the descriptor table, so the compiler cannot tell their address space and would use flat
// loads and stores (both wait counters, the LDS aperture check): they are global memory.
#ifdef SED_EMU
#define GATHER_GLOBAL
#else
#define GATHER_GLOBAL __attribute__((address_space(1)))
#endif

// One stream of a batch: the layout resident.py writes (include/sed_hip.h).
struct GatherDesc {
    const void* pool;              // row r starts at pool + r * stride input elements
    void* out;                     // dense (n_rows, len) output elements
    long long stride;              // input elements between pool rows
    int len;                       // elements per row
    int kind;
};
static_assert(sizeof(GatherDesc) == SED_GATHER_DESC_BYTES, "the descriptor layout of include/sed_hip.h");

template <int KIND> struct GatherKind;
template <> struct GatherKind<GATHER_I16_TO_F32> { typedef short in_t; typedef float out_t; };
template <> struct GatherKind<GATHER_F32> { typedef float in_t; typedef float out_t; };
template <> struct GatherKind<GATHER_U8_TO_F32> { typedef unsigned char in_t; typedef float out_t; };
template <> struct GatherKind<GATHER_U8> { typedef unsigned char in_t; typedef unsigned char out_t; };

__device__ __forceinline__ float gather_cvt(short x, float*) { return (float)x * (1.0f / 32768.0f); }       // exact: |x| <= 2^15
__device__ __forceinline__ float gather_cvt(float x, float*) { return x; }
__device__ __forceinline__ float gather_cvt(unsigned char x, float*) { return (float)x; }
__device__ __forceinline__ unsigned char gather_cvt(unsigned char x, unsigned char*) { return x; }

__device__ __forceinline__ float gather_i16(unsigned w, int hi) { return (float)(short)(hi ? (w >> 16) : (w & 0xFFFFu)) * (1.0f / 32768.0f); }
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));      // (native vectors: HIP's uint4 / float4 classes cannot be assigned through
__device__ __forceinline__ f32x4 gather_i16x4(unsigned a, unsigned b) {     //  an address-space-qualified pointer)
    const f32x4 r = {gather_i16(a, 0), gather_i16(a, 1), gather_i16(b, 0), gather_i16(b, 1)};
    return r;
}
__device__ __forceinline__ f32x4 gather_u8x4(unsigned w) {
    const f32x4 r = {(float)(w & 0xFFu), (float)((w >> 8) & 0xFFu), (float)((w >> 16) & 0xFFu), (float)(w >> 24)};
    return r;
}

// 16 input bytes -> the output elements they hold, stored as 16-byte words at dst (16-byte aligned)
template <int KIND>
__device__ __forceinline__ void gather_store16(const u32x4 v, GATHER_GLOBAL typename GatherKind<KIND>::out_t* dst) {
    if (KIND == GATHER_I16_TO_F32) {
        GATHER_GLOBAL f32x4* d = (GATHER_GLOBAL f32x4*)dst;
        d[0] = gather_i16x4(v.x, v.y);
        d[1] = gather_i16x4(v.z, v.w);
    } else if (KIND == GATHER_U8_TO_F32) {
        GATHER_GLOBAL f32x4* d = (GATHER_GLOBAL f32x4*)dst;
        d[0] = gather_u8x4(v.x); d[1] = gather_u8x4(v.y); d[2] = gather_u8x4(v.z); d[3] = gather_u8x4(v.w);
    } else {
        *(GATHER_GLOBAL u32x4*)dst = v;
    }
}

// elements [e0, e1) of one row; e0 is a multiple of GATHER_CHUNK
template <int KIND>
__device__ __forceinline__ void gather_chunk(const void* src_row, void* dst_row, int e0, int e1) {
    typedef typename GatherKind<KIND>::in_t in_t;
    typedef typename GatherKind<KIND>::out_t out_t;
    constexpr int VE = 16 / (int)sizeof(in_t);                      // elements per 16 input bytes
    constexpr int NIT = GATHER_CHUNK / VE / GATHER_THREADS;         // 16-byte loads per lane: 2 (int16), 4 (fp32), 1 (uint8)
    static_assert(NIT >= 1 && NIT * VE * GATHER_THREADS == GATHER_CHUNK, "a chunk is a whole number of passes");
    const GATHER_GLOBAL in_t* src = (const GATHER_GLOBAL in_t*)src_row + e0;
    GATHER_GLOBAL out_t* dst = (GATHER_GLOBAL out_t*)dst_row + e0;
    const int n = e1 - e0, tid = threadIdx.x;
    int done = 0;
    if (((((uintptr_t)src_row) | ((uintptr_t)dst_row)) & 15) == 0) {      // uniform: both rows (and so both chunks) 16-byte aligned
        const int nvec = n / VE;
        if (nvec > 0) {
            u32x4 v[NIT];
#pragma unroll
            for (int k = 0; k < NIT; ++k) {                         // every load in flight before the first store
                const int i = tid + GATHER_THREADS * k;
                v[k] = ((const GATHER_GLOBAL u32x4*)src)[i < nvec ? i : nvec - 1];
            }
#pragma unroll
            for (int k = 0; k < NIT; ++k) {
                const int i = tid + GATHER_THREADS * k;
                if (i < nvec) gather_store16<KIND>(v[k], dst + (size_t)i * VE);
            }
        }
        done = nvec * VE;
    }
    for (int i = done + tid; i < n; i += GATHER_THREADS) dst[i] = gather_cvt(src[i], (out_t*)nullptr);
}

__global__ __launch_bounds__(GATHER_THREADS) void batch_gather_kernel(const GatherDesc* __restrict__ desc, int n_streams,
                                                                      const int* __restrict__ idx, int chunks_per_row) {
    const int row = blockIdx.x / chunks_per_row;
    int c = blockIdx.x - row * chunks_per_row, s = 0, len = 0;
    for (; s < n_streams; ++s) {                                    // which stream this chunk of the row belongs to (uniform)
        len = desc[s].len;
        const int nc = (len + GATHER_CHUNK - 1) / GATHER_CHUNK;
        if (c < nc) break;
        c -= nc;
    }
    if (s == n_streams) return;
    const GatherDesc d = desc[s];
    const long long r = idx[row];                                   // one read per workgroup
    const int e0 = c * GATHER_CHUNK, e1 = min(len, e0 + GATHER_CHUNK);
    switch (d.kind) {
    case GATHER_I16_TO_F32:
        gather_chunk<GATHER_I16_TO_F32>((const short*)d.pool + r * d.stride, (float*)d.out + (size_t)row * len, e0, e1);
        break;
    case GATHER_F32:
        gather_chunk<GATHER_F32>((const float*)d.pool + r * d.stride, (float*)d.out + (size_t)row * len, e0, e1);
        break;
    case GATHER_U8_TO_F32:
        gather_chunk<GATHER_U8_TO_F32>((const unsigned char*)d.pool + r * d.stride, (float*)d.out + (size_t)row * len, e0, e1);
        break;
    case GATHER_U8:
        gather_chunk<GATHER_U8>((const unsigned char*)d.pool + r * d.stride, (unsigned char*)d.out + (size_t)row * len, e0, e1);
        break;
    default:
        break;
    }
}

// desc: n_streams (1..SED_GATHER_MAX_STREAMS) 32-byte descriptors in device memory; idx: n_rows int32 pool rows in device memory;
// chunks_per_row = sum over the streams of ceil(len / SED_GATHER_CHUNK), which the caller knows from the table it built.
SED_API int sed_batch_gather(const void* desc, int n_streams, const int* idx, int n_rows, int chunks_per_row, void* stream) {
    if (n_rows <= 0) return SED_OK;
    if (!desc || !idx || n_streams < 1 || n_streams > SED_GATHER_MAX_STREAMS || chunks_per_row < 1) return SED_ERR_ARG;
    if ((long long)n_rows * chunks_per_row >= (1ll << 31)) return SED_ERR_UNSUPPORTED;
    SED_LAUNCH(batch_gather_kernel, dim3((unsigned)(n_rows * chunks_per_row)), dim3(GATHER_THREADS), 0, (hipStream_t)stream,
               (const GatherDesc*)desc, n_streams, idx, chunks_per_row);
    return sed_check_launch();
}
