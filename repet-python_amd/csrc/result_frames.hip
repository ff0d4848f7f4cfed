// The spectra of a tensor call (repet_ctx_request_frames): what an offline pipeline decided in the time-frequency plane, read
// behind the pass that decided it, while its workspaces still hold it. The contract is the live handle's (frames.hip), per bin
// and in fp32:
//   mixture     V itself, as the forward kernel stored it
//   background  the magnitude of the masked bin AS THE VARIANT'S INVERSE STFT FETCHES IT, by magnitude() (common.h). A pipeline
//               leaves its masked spectrum in one of three forms (repet_ctx_last_spectrum_form):
//                 0  X masked in place                       |X|
//                 1  X and a mask plane Mk                    |(x.re * m, x.im * m)|, the products by mul_rounded as in the
//                                                             inverse kernels (stft.hip, stft_reg.hip: MASKED == 1)
//                 2  X, the repeating-segment model Wm and    the same with m = soft_mask(|X|, Wm[t mod period], f, cutoff), the
//                    the clips' periods                       expression of stft_reg.hip's MASKED == 2 (restated here: sharing a
//                                                             function would move the inverse kernel's code; tests/
//                                                             test_gpu_result_frames.py holds the two together through the
//                                                             waveform's own reference)
//               where the mask is 1 -- the high-pass bins -- the products are exact and the background equals the mixture to
//               the bit in every form
//   foreground  mixture - background, 0 where a rounding made that negative (NaN stays NaN)
// A frame at or past its clip's own frame count (a ragged batch) is zero in all three, whatever the rows hold -- they are not
// read; a warm-up frame of simonline has background 0 and foreground = mixture.
// One wavefront per (clip, frame, channel) in the frames kernel, four in the bands kernel (each takes every fourth band); a lane
// owns four consecutive bins of a 256-bin block: one 16-byte load of V, two of X and one of the plane or the model row. Rows are
// FS-padded (a multiple of 32 bins), so the loads never leave a row; only bins below F are stored or summed. Every bound is a
// host argument: the rows read are below `live`, the pass's own frame count, whatever the device tables say -- the clip-length
// table of a ragged batch can only lower it, and a period read from the device is reduced into the model's rows.
#include "engine.h"

namespace repet_eng {
namespace {

constexpr int kFrameDead = 0, kFrameWarm = 1, kFrameLive = 2;

// repet_frame_count's arithmetic, for the lengths a ragged batch keeps on the device
__device__ __forceinline__ int64_t grid_frames(int64_t n, int W, int H, int centred) {
    const int64_t num = centred ? n + 2 * (int64_t)(W / 2) - W : n - W;
    const int64_t q = num >= 0 ? (num + H - 1) / H : -((-num) / H);
    return q + 1;
}

// what frame t is to `clip` (uniform per wavefront: the clip is the workgroup's)
__device__ __forceinline__ int frame_state(const ResultFrameArgs& a, int clip, int64_t t) {
    int64_t live = a.live;
    if (a.lengths_dev) {
        const int64_t own = grid_frames(a.lengths_dev[clip], a.W, a.H, a.centred);
        live = own < live ? (own > 0 ? own : 0) : live;
    }
    return t >= live ? kFrameDead : (t < a.warm ? kFrameWarm : kFrameLive);
}

struct FrameRows { const float* V; const float2* X; const float* M; const float* Wr; };

// the rows of (clip, channel c, frame t); nothing is read here but the clip's period, and that only for a live frame of form 2
__device__ __forceinline__ FrameRows frame_rows(const ResultFrameArgs& a, int clip, int c, int64_t t, int state) {
    const int64_t row = clip * a.spec_stride + c * a.chan_stride + t * a.FS;
    FrameRows r{a.V + row, a.X + row, nullptr, nullptr};
    if (state != kFrameLive) return r;
    if (a.form == 1) r.M = a.Mk + row;
    if (a.form == 2) {
        int period = a.periods[clip];
        period = period < 1 ? 1 : period;
        int64_t q = t % period;
        q = q < a.model_rows ? q : a.model_rows - 1;               // (a period is at most model_rows - 1: never taken)
        r.Wr = a.model + clip * a.model_batch_stride + c * a.model_chan_stride + q * a.FS;
    }
    return r;
}

// the selected signal of bins [k, k + 4) of one row (k a multiple of 4 below FS)
__device__ __forceinline__ void result_group(const ResultFrameArgs& a, const FrameRows& r, int state, int k, float m[4]) {
    m[0] = m[1] = m[2] = m[3] = 0.f;
    if (state == kFrameDead) return;
    const float4 v = *reinterpret_cast<const float4*>(r.V + k);
    const float mix[4] = {v.x, v.y, v.z, v.w};
    if (a.which == REPET_OUT_MIXTURE) {
        for (int j = 0; j < 4; ++j) m[j] = mix[j];
        return;
    }
    float bg[4] = {0.f, 0.f, 0.f, 0.f};
    if (state == kFrameLive) {
        const float4 xa = *reinterpret_cast<const float4*>(r.X + k), xb = *reinterpret_cast<const float4*>(r.X + k + 2);
        const float2 x[4] = {make_float2(xa.x, xa.y), make_float2(xa.z, xa.w), make_float2(xb.x, xb.y), make_float2(xb.z, xb.w)};
        if (a.form == 0) {
            for (int j = 0; j < 4; ++j) bg[j] = magnitude(x[j]);
        } else {
            float mk[4];
            if (a.form == 1) {
                const float4 p = *reinterpret_cast<const float4*>(r.M + k);
                mk[0] = p.x; mk[1] = p.y; mk[2] = p.z; mk[3] = p.w;
            } else {
                const float4 w = *reinterpret_cast<const float4*>(r.Wr + k);
                const float wm[4] = {w.x, w.y, w.z, w.w};
                for (int j = 0; j < 4; ++j) mk[j] = soft_mask(magnitude(x[j]), wm[j], k + j, a.cutoff);
            }
            for (int j = 0; j < 4; ++j) bg[j] = magnitude(make_float2(mul_rounded(x[j].x, mk[j]), mul_rounded(x[j].y, mk[j])));
        }
    }
    for (int j = 0; j < 4; ++j) {
        const float d = mix[j] - bg[j];
        m[j] = a.which == REPET_OUT_BACKGROUND ? bg[j] : (d < 0.f ? 0.f : d);
    }
}

struct ResultDst { float* p; int64_t s_clip, s_frame, s_channel, s_bin; };

__global__ __launch_bounds__(64) void result_frames_kernel(ResultFrameArgs a, ResultDst d) {
    const int clip = blockIdx.y, lane = threadIdx.x;
    const int64_t t = blockIdx.x / a.C;
    const int c = (int)(blockIdx.x - t * a.C);
    const int state = frame_state(a, clip, t);
    const FrameRows r = frame_rows(a, clip, c, t, state);
    float* out = d.p + clip * d.s_clip + t * d.s_frame + c * d.s_channel;
    // bins side by side and the row's first on a 16-byte boundary: one store per lane
    const bool vec = d.s_bin == 1 && !(reinterpret_cast<uintptr_t>(out) & 15);
    for (int k = 4 * lane; k < a.F; k += 256) {
        float m[4];
        result_group(a, r, state, k, m);
        if (vec && k + 4 <= a.F) {
            *reinterpret_cast<float4*>(out + k) = make_float4(m[0], m[1], m[2], m[3]);
        } else {
            for (int j = 0; j < 4; ++j)
                if (k + j < a.F) out[(k + j) * d.s_bin] = m[j];
        }
    }
}

struct ResultEdges { int32_t n; int32_t at[REPET_MAX_BANDS + 1]; };

constexpr int kBandWaves = 4;

// The reduction shape of online_bands_kernel (frames.hip): a lane adds the squares of its own bins of the band in bin order,
// block of 256 bins after block; the wave folds the 64 sums by __shfl_xor; lane 0 stores. No atomics: the same bits from every
// call. A band is one wave's from its first load to its store.
__global__ __launch_bounds__(64 * kBandWaves) void result_bands_kernel(ResultFrameArgs a, ResultEdges e, double* __restrict__ dst,
                                                                       int64_t clip_stride) {
    const int clip = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = blockIdx.x / a.C;
    const int c = (int)(blockIdx.x - t * a.C);
    const int state = frame_state(a, clip, t);
    const FrameRows r = frame_rows(a, clip, c, t, state);
    double* out = dst + clip * clip_stride + (t * a.C + c) * e.n;
    for (int b = wave; b < e.n; b += kBandWaves) {
        const int lo = e.at[b], hi = e.at[b + 1];                      // 0 <= lo <= hi <= F (checked on the host)
        double acc = 0.0;
        if (state != kFrameDead) {
            for (int base = lo & ~255; base < hi; base += 256) {
                const int k = base + 4 * lane;
                if (k + 4 <= lo || k >= hi) continue;
                float m[4];
                result_group(a, r, state, k, m);
                for (int j = 0; j < 4; ++j)
                    if (k + j >= lo && k + j < hi) acc += (double)m[j] * (double)m[j];
            }
        }
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) out[b] = acc;
    }
}

bool result_launchable(const ResultFrameArgs& a, int32_t n_clips) {
    if (!a.V || !a.X || a.C <= 0 || a.F <= 0 || a.FS < a.F || (a.FS & 3) || n_clips > 65535 || a.n_frames * a.C > 0x7fffffff) return false;
    if (a.which < REPET_OUT_BACKGROUND || a.which > REPET_OUT_MIXTURE || a.live < 0 || a.chan_stride < a.live * a.FS) return false;
    if (a.form == 1 && !a.Mk) return false;
    if (a.form == 2 && (!a.model || !a.periods || a.model_rows < 1 || a.model_chan_stride < (int64_t)a.model_rows * a.FS)) return false;
    if (a.lengths_dev && (a.W < 2 || a.H < 1)) return false;
    return a.form >= 0 && a.form <= 2;
}

}  // namespace

hipError_t launch_result_frames(const ResultFrameArgs& a, int32_t n_clips, float* dst, const int64_t strides[4], hipStream_t s) {
    if (n_clips <= 0 || a.n_frames <= 0) return hipSuccess;
    if (!dst || !result_launchable(a, n_clips)) return hipErrorInvalidValue;
    const ResultDst d{dst, strides[0], strides[1], strides[2], strides[3]};
    result_frames_kernel<<<dim3((unsigned)(a.n_frames * a.C), (unsigned)n_clips), 64, 0, s>>>(a, d);
    return hipGetLastError();
}

hipError_t launch_result_bands(const ResultFrameArgs& a, int32_t n_clips, const int32_t* edges, int32_t n_bands, double* dst,
                               int64_t clip_stride, hipStream_t s) {
    if (n_clips <= 0 || a.n_frames <= 0) return hipSuccess;
    if (!dst || !edges || n_bands < 1 || n_bands > REPET_MAX_BANDS || !result_launchable(a, n_clips)) return hipErrorInvalidValue;
    ResultEdges e{};
    e.n = n_bands;
    for (int32_t k = 0; k <= n_bands; ++k) {
        if (edges[k] < 0 || edges[k] > a.F || (k > 0 && edges[k] < edges[k - 1])) return hipErrorInvalidValue;
        e.at[k] = edges[k];
    }
    result_bands_kernel<<<dim3((unsigned)(a.n_frames * a.C), (unsigned)n_clips), 64 * kBandWaves, 0, s>>>(a, e, dst, clip_stride);
    return hipGetLastError();
}

}  // namespace repet_eng
