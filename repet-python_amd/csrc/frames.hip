// The spectra of a streaming handle's last frames (repet_online_last_frames* / last_band_energies*): what a push decided in
// the time-frequency plane, read where the push left it. For every new frame of every slot the window that was current during
// the push still holds the mixture magnitudes (V, as the forward kernel stored them) and the masked spectrum (X after the mask
// kernel); nothing writes those rows before the next push. Per bin, in fp32:
//   mixture     V itself
//   background  |X| by magnitude() (common.h), the function the forward kernel formed V with: where the mask is 1 -- the
//               high-pass bins -- X is what it was and the background equals the mixture to the bit
//   foreground  mixture - background, 0 where a rounding made that negative (NaN stays NaN)
// A frame before its slot's own first frame (an idle or held slot: every frame) is zero in all three, whatever the rows hold;
// a warm-up frame has background 0 and foreground = mixture. Liveness comes from the slot table the push's own kernels read.
// The frames kernel runs one wavefront per (slot, frame, channel), the bands kernel four (each takes every fourth band); a lane owns four consecutive bins of a 256-bin block: one 16-byte
// load of V and two of X. Rows are FS-padded (a multiple of 32 bins, the pad bins zero), so the loads never leave a row; only
// bins below F are stored or summed. Every bound comes from the host's record of the push: nothing indexes from device data.
#include "engine.h"

namespace repet_eng {
namespace {

constexpr int kFrameDead = 0, kFrameWarm = 1, kFrameLive = 2;

// what frame t of the record is to `slot` (one uniform load per wavefront: the slot is the workgroup's)
__device__ __forceinline__ int frame_state(const FrameArgs& a, int slot, int64_t t) {
    const int64_t start = a.slot_start ? a.slot_start[slot] : 0;       // kSlotIdle / kSlotHeld: past every frame
    const int64_t own = a.frame0 + t - start;                          // the slot's own number of this frame
    return own < 0 ? kFrameDead : (own < a.warm ? kFrameWarm : kFrameLive);
}

// the selected signal of bins [k, k + 4) of one row (k a multiple of 4 below FS)
__device__ __forceinline__ void frame_group(const FrameArgs& a, const float* __restrict__ Vrow, const float2* __restrict__ Xrow, int state,
                                            int k, float m[4]) {
    m[0] = m[1] = m[2] = m[3] = 0.f;
    if (state == kFrameDead) return;
    const float4 v = *reinterpret_cast<const float4*>(Vrow + k);
    const float mix[4] = {v.x, v.y, v.z, v.w};
    if (a.which == REPET_OUT_MIXTURE) {
        for (int j = 0; j < 4; ++j) m[j] = mix[j];
        return;
    }
    float bg[4] = {0.f, 0.f, 0.f, 0.f};
    if (state == kFrameLive) {
        const float4 xa = *reinterpret_cast<const float4*>(Xrow + k), xb = *reinterpret_cast<const float4*>(Xrow + k + 2);
        bg[0] = magnitude(make_float2(xa.x, xa.y));
        bg[1] = magnitude(make_float2(xa.z, xa.w));
        bg[2] = magnitude(make_float2(xb.x, xb.y));
        bg[3] = magnitude(make_float2(xb.z, xb.w));
    }
    for (int j = 0; j < 4; ++j) {
        const float d = mix[j] - bg[j];
        m[j] = a.which == REPET_OUT_BACKGROUND ? bg[j] : (d < 0.f ? 0.f : d);
    }
}

struct FrameDst { float* p; int64_t s_stream, s_frame, s_channel, s_bin; };

__global__ __launch_bounds__(64) void online_frames_kernel(FrameArgs a, FrameDst d) {
    const int slot = blockIdx.y, lane = threadIdx.x;
    const int64_t t = blockIdx.x / a.C;
    const int c = (int)(blockIdx.x - t * a.C);
    const int state = frame_state(a, slot, t);
    const int64_t row = slot * a.spec + c * a.plane + t * a.FS;
    const float* Vrow = a.V + row;
    const float2* Xrow = a.X + row;
    float* out = d.p + slot * d.s_stream + t * d.s_frame + c * d.s_channel;
    // bins side by side and the row's first on a 16-byte boundary: one store per lane
    const bool vec = d.s_bin == 1 && !(reinterpret_cast<uintptr_t>(out) & 15);
    for (int k = 4 * lane; k < a.F; k += 256) {
        float m[4];
        frame_group(a, Vrow, Xrow, state, k, m);
        if (vec && k + 4 <= a.F) {
            *reinterpret_cast<float4*>(out + k) = make_float4(m[0], m[1], m[2], m[3]);
        } else {
            for (int j = 0; j < 4; ++j)
                if (k + j < a.F) out[(k + j) * d.s_bin] = m[j];
        }
    }
}

struct BandEdges { int32_t n; int32_t at[REPET_MAX_BANDS + 1]; };

constexpr int kBandWaves = 4;

// One fixed shape: a lane adds the squares of its own bins of the band in bin order, block of 256 bins after block; the wave
// folds the 64 sums by __shfl_xor; lane 0 stores. No atomics: the same bits from every call. A band is one wave's from its
// first load to its store; the workgroup's kBandWaves waves take the bands in turn and share nothing.
__global__ __launch_bounds__(64 * kBandWaves) void online_bands_kernel(FrameArgs a, BandEdges e, double* __restrict__ dst) {
    const int slot = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = blockIdx.x / a.C;
    const int c = (int)(blockIdx.x - t * a.C);
    const int state = frame_state(a, slot, t);
    const int64_t row = slot * a.spec + c * a.plane + t * a.FS;
    const float* Vrow = a.V + row;
    const float2* Xrow = a.X + row;
    double* out = dst + ((slot * a.n_frames + t) * a.C + c) * e.n;
    for (int b = wave; b < e.n; b += kBandWaves) {
        const int lo = e.at[b], hi = e.at[b + 1];                      // 0 <= lo <= hi <= F (checked on the host)
        double acc = 0.0;
        if (state != kFrameDead) {
            for (int base = lo & ~255; base < hi; base += 256) {
                const int k = base + 4 * lane;
                if (k + 4 <= lo || k >= hi) continue;
                float m[4];
                frame_group(a, Vrow, Xrow, state, k, m);
                for (int j = 0; j < 4; ++j)
                    if (k + j >= lo && k + j < hi) acc += (double)m[j] * (double)m[j];
            }
        }
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) out[b] = acc;
    }
}

static bool frames_launchable(const FrameArgs& a, int32_t n_streams) {
    return a.V && a.X && a.C > 0 && a.F > 0 && a.FS >= a.F && !(a.FS & 3) && n_streams <= 65535 && a.n_frames * a.C <= 0x7fffffff &&
           a.which >= REPET_OUT_BACKGROUND && a.which <= REPET_OUT_MIXTURE;
}

}  // namespace

hipError_t launch_online_frames(const FrameArgs& a, int32_t n_streams, float* dst, const int64_t strides[4], hipStream_t s) {
    if (n_streams <= 0 || a.n_frames <= 0) return hipSuccess;
    if (!dst || !frames_launchable(a, n_streams)) return hipErrorInvalidValue;
    const FrameDst d{dst, strides[0], strides[1], strides[2], strides[3]};
    online_frames_kernel<<<dim3((unsigned)(a.n_frames * a.C), (unsigned)n_streams), 64, 0, s>>>(a, d);
    return hipGetLastError();
}

hipError_t launch_online_bands(const FrameArgs& a, int32_t n_streams, const int32_t* edges, int32_t n_bands, double* dst, hipStream_t s) {
    if (n_streams <= 0 || a.n_frames <= 0) return hipSuccess;
    if (!dst || !edges || n_bands < 1 || n_bands > REPET_MAX_BANDS || !frames_launchable(a, n_streams)) return hipErrorInvalidValue;
    BandEdges e{};
    e.n = n_bands;
    for (int32_t k = 0; k <= n_bands; ++k) {
        if (edges[k] < 0 || edges[k] > a.F || (k > 0 && edges[k] < edges[k - 1])) return hipErrorInvalidValue;
        e.at[k] = edges[k];
    }
    online_bands_kernel<<<dim3((unsigned)(a.n_frames * a.C), (unsigned)n_streams), 64 * kBandWaves, 0, s>>>(a, e, dst);
    return hipGetLastError();
}

}  // namespace repet_eng
