// Device-side ingest and egress of caller tensors (torch tensors on a ROCm device, a C++ host's own buffers): the engine's
// fp32 interleaved planes are filled from, and its result is widened into, device memory of any layout the caller holds --
// (n_clips, n_samples, n_channels) with arbitrary non-negative element strides -- ordered on the caller's stream by events,
// with no host wait and no host bounce.
//   ingest  source (F64 / F32 / I16 / F16 / BF16, strided) -> audio [clip][n][c] fp32, and for F64 also audio_lo, the fp32
//           remainders: hi = (float)x, lo = (float)(x - (double)hi) -- exactly what narrow_f64 / split_part of hostio.hip
//           produce, so the planes equal a host upload's bit for bit. I16 is the raw (float) cast of narrow_i16; F16 / BF16
//           widen exactly. With a flag word it also notes a sample that is not finite (the refusal mode reads it).
//   egress  out [clip][n][c] fp32 -> destination (F64: (double)v as widen_f32 does, F32, or I16 / F16 / BF16: the inverse of
//           the ingest's cast, never a rescale -- the value rounded ONCE to nearest, ties to even, see narrow()), strided.
// Both are bandwidth kernels: every thread owns a few consecutive elements of the interleaved side, which it reads or writes
// with one vector access, so that each 128-byte line of that side is moved whole by one instruction of one wave; the strided
// side takes element accesses, vector ones when it is the same dense layout and aligned.
#include "engine.h"

namespace repet {
namespace {

constexpr int kIoThreads = 256;

struct IoGeo {
    int64_t count;                 // n_clips * n_samples * n_channels
    int64_t n_samples;
    int32_t n_channels;
    int64_t s_clip, s_sample, s_channel;   // element strides of the strided side
};

// element i of the interleaved side -> offset on the strided side (i is the first of a thread's run; the rest step along)
struct Walker {
    int64_t b, n, c, off;
    __device__ Walker(const IoGeo& g, int64_t i) {
        c = i % g.n_channels;
        const int64_t t = i / g.n_channels;
        n = t % g.n_samples;
        b = t / g.n_samples;
        off = b * g.s_clip + n * g.s_sample + c * g.s_channel;
    }
    __device__ void next(const IoGeo& g) {
        if (++c < g.n_channels) { off += g.s_channel; return; }
        c = 0;
        if (++n < g.n_samples) { off += g.s_sample - (int64_t)(g.n_channels - 1) * g.s_channel; return; }
        n = 0; ++b;
        off = b * g.s_clip;
    }
};

template <typename T> struct Src;
template <> struct Src<double> { static __device__ double load(const double* p) { return *p; } };
template <> struct Src<float> { static __device__ float load(const float* p) { return *p; } };
template <> struct Src<int16_t> { static __device__ float load(const int16_t* p) { return (float)*p; } };
struct Half { uint16_t bits; };
__device__ inline float h2f(uint16_t bits) { return (float)__builtin_bit_cast(_Float16, bits); }
struct BHalf { uint16_t bits; };
template <> struct Src<Half> { static __device__ float load(const Half* p) { return h2f(p->bits); } };
template <> struct Src<BHalf> { static __device__ float load(const BHalf* p) { return __uint_as_float((uint32_t)p->bits << 16); } };

template <typename T> __device__ inline bool not_finite(T v);
template <> __device__ inline bool not_finite<double>(double v) { return !(fabs(v) <= 1.7976931348623157e308); }
template <> __device__ inline bool not_finite<float>(float v) { return !(fabsf(v) <= 3.402823466e38f); }

// one sample -> (hi, lo); lo only for float64 sources
template <typename T> __device__ inline void split1(const T* src, float& hi, float& lo, bool& bad, bool check) {
    auto x = Src<T>::load(src);
    if constexpr (std::is_same<T, double>::value) {
        hi = (float)x;
        lo = (float)(x - (double)hi);
        if (check) bad |= not_finite(x);
    } else {
        hi = x; lo = 0.f;
        if (check && !std::is_same<T, int16_t>::value) bad |= not_finite(hi);
    }
}

// dense source (its layout IS the interleaved one) aligned for a 4-element vector load
template <typename T> __device__ inline void load4_dense(const T* src, float (&hi)[4], float (&lo)[4]);
template <> __device__ inline void load4_dense<double>(const double* src, float (&hi)[4], float (&lo)[4]) {
    const double2 a = reinterpret_cast<const double2*>(src)[0], b = reinterpret_cast<const double2*>(src)[1];
    const double x[4] = {a.x, a.y, b.x, b.y};
#pragma unroll
    for (int k = 0; k < 4; ++k) { hi[k] = (float)x[k]; lo[k] = (float)(x[k] - (double)hi[k]); }
}
// (the float64 check is on the double itself: a finite sample above FLT_MAX narrows to inf but is not refused, as on the host)
__device__ inline bool dense_not_finite(const double* src) {
    const double2 a = reinterpret_cast<const double2*>(src)[0], b = reinterpret_cast<const double2*>(src)[1];
    return not_finite(a.x) || not_finite(a.y) || not_finite(b.x) || not_finite(b.y);
}
template <> __device__ inline void load4_dense<float>(const float* src, float (&hi)[4], float (&lo)[4]) {
    const float4 a = *reinterpret_cast<const float4*>(src);
    hi[0] = a.x; hi[1] = a.y; hi[2] = a.z; hi[3] = a.w;
#pragma unroll
    for (int k = 0; k < 4; ++k) lo[k] = 0.f;
}
template <> __device__ inline void load4_dense<int16_t>(const int16_t* src, float (&hi)[4], float (&lo)[4]) {
    const short4 a = *reinterpret_cast<const short4*>(src);
    hi[0] = (float)a.x; hi[1] = (float)a.y; hi[2] = (float)a.z; hi[3] = (float)a.w;
#pragma unroll
    for (int k = 0; k < 4; ++k) lo[k] = 0.f;
}
template <> __device__ inline void load4_dense<Half>(const Half* src, float (&hi)[4], float (&lo)[4]) {
    const ushort4 a = *reinterpret_cast<const ushort4*>(src);
    hi[0] = h2f(a.x); hi[1] = h2f(a.y);
    hi[2] = h2f(a.z); hi[3] = h2f(a.w);
#pragma unroll
    for (int k = 0; k < 4; ++k) lo[k] = 0.f;
}
template <> __device__ inline void load4_dense<BHalf>(const BHalf* src, float (&hi)[4], float (&lo)[4]) {
    const ushort4 a = *reinterpret_cast<const ushort4*>(src);
    hi[0] = __uint_as_float((uint32_t)a.x << 16); hi[1] = __uint_as_float((uint32_t)a.y << 16);
    hi[2] = __uint_as_float((uint32_t)a.z << 16); hi[3] = __uint_as_float((uint32_t)a.w << 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) lo[k] = 0.f;
}

// Four consecutive interleaved elements per thread: one dwordx4 store per plane, 1 KiB per wave instruction.
// kRagged (repet_ctx_upload_device_ragged): clip b has lengths[b] live samples. A run that lies below its clip's length is today's
// conversion by today's code; a run at or behind it stores zeros and loads nothing; the run a length cuts (a length times the
// channel count need not be a multiple of four) goes element by element, loading the live elements only. The non-finite note
// therefore looks at live samples alone.
template <typename T, bool kRagged = false>
__device__ inline void ingest_body(const T* __restrict__ src, IoGeo g, int dense, float* __restrict__ hi_out,
                                   float* __restrict__ lo_out, unsigned int* nonfinite, const int64_t* __restrict__ lengths = nullptr) {
    constexpr bool kSplit = std::is_same<T, double>::value;
    const int64_t i0 = ((int64_t)blockIdx.x * kIoThreads + threadIdx.x) * 4;
    if (i0 >= g.count) return;
    const bool check = nonfinite != nullptr;
    bool bad = false;
    float hi[4], lo[4];
    if constexpr (kRagged) {
        const int m = g.count - i0 < 4 ? (int)(g.count - i0) : 4;
        // (clip, sample, channel) of the run's first element: 32-bit divisions where the plane allows them
        int64_t b, n;
        int32_t c;
        if (g.count <= 0xffffffffll) {
            const uint32_t t = (uint32_t)i0 / (uint32_t)g.n_channels;
            c = (int32_t)((uint32_t)i0 - t * (uint32_t)g.n_channels);
            b = t / (uint32_t)g.n_samples;
            n = t - (uint32_t)b * (uint32_t)g.n_samples;
        } else {
            const int64_t t = i0 / g.n_channels;
            c = (int32_t)(i0 - t * g.n_channels);
            b = t / g.n_samples;
            n = t - b * g.n_samples;
        }
        bool live[4];
        int n_live = 0;
        int64_t len = lengths[b];                                 // (loaded again only where the run enters the next clip)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            live[k] = false;
            if (k < m) {
                live[k] = n < len;
                n_live += live[k] ? 1 : 0;
                if (++c == g.n_channels) {
                    c = 0;
                    if (++n == g.n_samples) {
                        n = 0; ++b;
                        if (k < m - 1) len = lengths[b];
                    }
                }
            }
        }
        if (n_live < 4) {                                         // (all four live: the run is the equal-length path's, below)
            if (m == 4 && n_live == 0) {
                *reinterpret_cast<float4*>(hi_out + i0) = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (kSplit) *reinterpret_cast<float4*>(lo_out + i0) = make_float4(0.f, 0.f, 0.f, 0.f);
                return;
            }
            Walker w(g, i0);
            for (int k = 0; k < m; ++k) {
                float h = 0.f, l = 0.f;
                if (live[k]) split1<T>(src + w.off, h, l, bad, check);
                hi_out[i0 + k] = h;
                if constexpr (kSplit) lo_out[i0 + k] = l;
                if (k < m - 1) w.next(g);
            }
            if (bad) *nonfinite = 1u;
            return;
        }
    }
    if (i0 + 4 <= g.count) {
        if (dense) {
            load4_dense<T>(src + i0, hi, lo);
            if (check) {
                if constexpr (kSplit) bad |= dense_not_finite(src + i0);
                else if constexpr (!std::is_same<T, int16_t>::value) {
                    for (int k = 0; k < 4; ++k) bad |= not_finite(hi[k]);
                }
            }
        } else {
            Walker w(g, i0);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                split1<T>(src + w.off, hi[k], lo[k], bad, check);
                if (k < 3) w.next(g);
            }
        }
        *reinterpret_cast<float4*>(hi_out + i0) = make_float4(hi[0], hi[1], hi[2], hi[3]);
        if constexpr (kSplit) *reinterpret_cast<float4*>(lo_out + i0) = make_float4(lo[0], lo[1], lo[2], lo[3]);
    } else {                                                      // the tail of the plane: one thread, element by element
        Walker w(g, i0);
        for (int64_t i = i0; i < g.count; ++i) {
            float h, l;
            split1<T>(src + w.off, h, l, bad, check);
            hi_out[i] = h;
            if constexpr (kSplit) lo_out[i] = l;
            w.next(g);
        }
    }
    if (bad) *nonfinite = 1u;                                     // (every writer stores the same value)
}

// The last store of an emission: the float64 value the engine holds -> the destination's type. A destination dtype is the
// inverse of the same source dtype: a cast, never a rescale (I16 ingest is the raw (float) cast, so I16 egress returns the
// same units: a +-1.0 float stream emitted as int16 is 0 / +-1).
//   F64 / F32  the C++ conversion, as ever.
//   F16 / BF16 the nearest value of the format, ties to even, rounded ONCE from float64 (through float32 it would be rounded
//              twice): beyond the largest finite +-inf, subnormals produced, NaN a quiet NaN, the sign of zero kept. An integer
//              sequence on the double's bits, E exponent and M fraction bits (binary16: 5, 10; bfloat16: 8, 7): the
//              significand shifted down to the format's last place -- further below its smallest normal --, then
//              incremented where the bits shifted out are above half a place, or exactly half with an odd last place; the
//              carry of that increment runs into the exponent field by itself, up to infinity.
//   I16        round to nearest, ties to even (v_rndne_f64), saturated to [-32768, 32767]; NaN is 0.
template <int E, int M> __host__ __device__ inline uint16_t round_f64_bits(double v) {
    constexpr int kMax = (1 << E) - 1, kBias = (1 << (E - 1)) - 1;
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t sign = (uint32_t)(u >> 48) & 0x8000u;
    const int e = (int)(u >> 52) & 0x7ff;
    const uint64_t frac = u & 0xfffffffffffffull;
    if (e == 0x7ff) return (uint16_t)(sign | (uint32_t)(kMax << M) | (frac ? 1u << (M - 1) : 0u));
    const int te = e - 1023 + kBias;                              // the exponent field of a normal result
    if (te >= kMax) return (uint16_t)(sign | (uint32_t)(kMax << M));
    const uint64_t sig = frac | (e ? 1ull << 52 : 0ull);
    int sh = 52 - M + (te >= 1 ? 0 : 1 - te);                     // (54 and more: below half the smallest subnormal, all alike)
    sh = sh < 54 ? sh : 54;
    uint32_t r = (te >= 1 ? (uint32_t)(te - 1) << M : 0u) + (uint32_t)(sig >> sh);      // (the hidden bit completes the field)
    const uint64_t rem = sig & ((1ull << sh) - 1), half = 1ull << (sh - 1);
    r += rem > half || (rem == half && (r & 1u)) ? 1u : 0u;
    return (uint16_t)(sign | r);
}

template <typename T> __device__ inline T narrow(double v) { return (T)v; }
template <> __device__ inline int16_t narrow<int16_t>(double v) {
    return (int16_t)(int32_t)(v != v ? 0.0 : fmin(fmax(rint(v), -32768.0), 32767.0));
}
template <> __device__ inline Half narrow<Half>(double v) { return Half{round_f64_bits<5, 10>(v)}; }
template <> __device__ inline BHalf narrow<BHalf>(double v) { return BHalf{round_f64_bits<8, 7>(v)}; }

__device__ inline uint32_t bits16(int16_t v) { return (uint16_t)v; }
__device__ inline uint32_t bits16(Half v) { return v.bits; }
__device__ inline uint32_t bits16(BHalf v) { return v.bits; }

// Elements per thread of the kernels that write a 16-bit type: four, an 8-byte store per lane on a dense destination beside the
// 16-byte loads of the fp32 planes. (Eight -- a 16-byte store -- costs devio_emit_* 74 VGPRs against the 48 of devio_emit_f32 and
// of the four-element form: six waves per SIMD instead of eight; profiles/HISTORY.md.)
constexpr int kEpt16 = 4;

// EPT consecutive fp32 values by one vector load (2: a float2; 4: a float4), p aligned for it
template <int EPT> __device__ inline void load_run(const float* p, float (&v)[EPT]) {
    if constexpr (EPT == 2) { const float2 a = *reinterpret_cast<const float2*>(p); v[0] = a.x; v[1] = a.y; }
    else { const float4 a = *reinterpret_cast<const float4*>(p); v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; }
}

// EPT consecutive elements of a dense destination by ONE vector store (F64: double2, F32: float4, 16-bit types: four elements
// in a uint2), p aligned for it
template <typename T, int EPT> __device__ inline void store_run(T* p, const T (&v)[EPT]) {
    if constexpr (sizeof(T) == 8) *reinterpret_cast<double2*>(p) = make_double2(v[0], v[1]);
    else if constexpr (sizeof(T) == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *reinterpret_cast<uint2*>(p) = make_uint2(bits16(v[0]) | bits16(v[1]) << 16, bits16(v[2]) | bits16(v[3]) << 16);
}

// Egress: EPT consecutive interleaved elements per thread, read with one vector load (F64: 2 -> float2 in, double2 out;
// F32: 4 -> float4 in and out; I16 / F16 / BF16: 4 -> float4 in, 8 bytes out), so that the interleaved side and a dense
// destination move whole lines per instruction. (An fp32 value widens exactly: narrow() rounds it once.)
template <typename T, int EPT>
__device__ inline void egress_body(const float* __restrict__ in, IoGeo g, int dense, T* __restrict__ dst) {
    const int64_t i0 = ((int64_t)blockIdx.x * kIoThreads + threadIdx.x) * EPT;
    if (i0 >= g.count) return;
    if (i0 + EPT <= g.count) {
        float v[EPT];
        load_run<EPT>(in + i0, v);
        if (dense) {
            T t[EPT];
#pragma unroll
            for (int k = 0; k < EPT; ++k) t[k] = narrow<T>((double)v[k]);
            store_run<T, EPT>(dst + i0, t);
        } else {
            Walker w(g, i0);
#pragma unroll
            for (int k = 0; k < EPT; ++k) {
                dst[w.off] = narrow<T>((double)v[k]);
                if (k < EPT - 1) w.next(g);
            }
        }
    } else {
        Walker w(g, i0);
        for (int64_t i = i0; i < g.count; ++i) { dst[w.off] = narrow<T>((double)in[i]); w.next(g); }
    }
}

// stable names, one per source / destination type (rocprofv3 rows)
__global__ __launch_bounds__(kIoThreads) void devio_ingest_f64(const double* src, IoGeo g, int dense, float* hi, float* lo, unsigned int* nf) { ingest_body<double>(src, g, dense, hi, lo, nf); }
__global__ __launch_bounds__(kIoThreads) void devio_ingest_f32(const float* src, IoGeo g, int dense, float* hi, float* lo, unsigned int* nf) { ingest_body<float>(src, g, dense, hi, lo, nf); }
__global__ __launch_bounds__(kIoThreads) void devio_ingest_i16(const int16_t* src, IoGeo g, int dense, float* hi, float* lo, unsigned int* nf) { ingest_body<int16_t>(src, g, dense, hi, lo, nf); }
__global__ __launch_bounds__(kIoThreads) void devio_ingest_f16(const Half* src, IoGeo g, int dense, float* hi, float* lo, unsigned int* nf) { ingest_body<Half>(src, g, dense, hi, lo, nf); }
__global__ __launch_bounds__(kIoThreads) void devio_ingest_bf16(const BHalf* src, IoGeo g, int dense, float* hi, float* lo, unsigned int* nf) { ingest_body<BHalf>(src, g, dense, hi, lo, nf); }
__global__ __launch_bounds__(kIoThreads) void devio_ingest_ragged_f64(const double* src, IoGeo g, int dense, float* hi, float* lo, unsigned int* nf, const int64_t* len) { ingest_body<double, true>(src, g, dense, hi, lo, nf, len); }
__global__ __launch_bounds__(kIoThreads) void devio_ingest_ragged_f32(const float* src, IoGeo g, int dense, float* hi, float* lo, unsigned int* nf, const int64_t* len) { ingest_body<float, true>(src, g, dense, hi, lo, nf, len); }
__global__ __launch_bounds__(kIoThreads) void devio_ingest_ragged_i16(const int16_t* src, IoGeo g, int dense, float* hi, float* lo, unsigned int* nf, const int64_t* len) { ingest_body<int16_t, true>(src, g, dense, hi, lo, nf, len); }
__global__ __launch_bounds__(kIoThreads) void devio_ingest_ragged_f16(const Half* src, IoGeo g, int dense, float* hi, float* lo, unsigned int* nf, const int64_t* len) { ingest_body<Half, true>(src, g, dense, hi, lo, nf, len); }
__global__ __launch_bounds__(kIoThreads) void devio_ingest_ragged_bf16(const BHalf* src, IoGeo g, int dense, float* hi, float* lo, unsigned int* nf, const int64_t* len) { ingest_body<BHalf, true>(src, g, dense, hi, lo, nf, len); }
__global__ __launch_bounds__(kIoThreads) void devio_egress_f64(const float* in, IoGeo g, int dense, double* dst) { egress_body<double, 2>(in, g, dense, dst); }
__global__ __launch_bounds__(kIoThreads) void devio_egress_f32(const float* in, IoGeo g, int dense, float* dst) { egress_body<float, 4>(in, g, dense, dst); }
__global__ __launch_bounds__(kIoThreads) void devio_egress_i16(const float* in, IoGeo g, int dense, int16_t* dst) { egress_body<int16_t, kEpt16>(in, g, dense, dst); }
__global__ __launch_bounds__(kIoThreads) void devio_egress_f16(const float* in, IoGeo g, int dense, Half* dst) { egress_body<Half, kEpt16>(in, g, dense, dst); }
__global__ __launch_bounds__(kIoThreads) void devio_egress_bf16(const float* in, IoGeo g, int dense, BHalf* dst) { egress_body<BHalf, kEpt16>(in, g, dense, dst); }

// Emission of the streaming handle, and the selected result of an offline context: what was emitted as background (`bg`, fp32
// [S][n][C] dense), as foreground (input - background) or as mixture (the input itself, aligned with what was emitted), into
// one or two strided destinations in ONE pass. The input is read where the engine holds it: fp32 samples `hi` and, where
// present, their fp32 remainders `lo`, stream s at s * in_stream floats. In float64: mixture = hi + lo (exact),
// foreground = mixture - bg (rounded once); an F32 / I16 / F16 / BF16 destination takes that value rounded once more, by
// narrow(): the destination dtype is a property of the last store alone. A sample of stream s is
// LIVE from handle sample slot_start[s] * hop on (pos0: handle sample of the emission's first one; no table: always); every
// other sample is zero in all three signals by a select, so NaN in an idle slot's share of a chunk never shows.
// EPT consecutive interleaved elements per thread as in egress_body: vector accesses on bg, on hi / lo where the run lies in
// one stream and is aligned, on a dense destination.
// Background gain (`gain` != 0; 0 is the path above, untouched): foreground = fma(-a, bg, x) in float64 with a an fp32 value, so
// a * bg is exact and the foreground is x - a * bg rounded once. kGainScalar: a = `a` for every sample (offline contexts).
// kGainTables: per stream s, for its sample j (0-based within this emission): a = a_tgt[s] where j + 1 >= ramp (a select), else
// the fade fma(a_tgt[s] - a_cur[s], (j + 1) / ramp, a_cur[s]); a slot whose two entries are equal fades nowhere.
constexpr int32_t kGainScalar = 1, kGainTables = 2;
struct EmitOut { void* p; int64_t s_clip, s_sample, s_channel; int32_t which, dense; };
struct EmitArgs {
    const float* bg; const float* hi; const float* lo;
    int64_t in_stream, count, per, n_samples;
    const int64_t* slot_start; int64_t pos0, hop;
    int32_t n_channels, n_out;
    EmitOut out[2];
    const float* a_cur; const float* a_tgt; int64_t ramp; float a; int32_t gain;
    const float* bg_fg;             // (nullable) the background the FOREGROUND is formed from, laid out like bg: a live handle's shaped one
    // (nullable) a ragged offline batch: stream s is live below sample live_len[s] of the emission. At and behind it every signal
    // is zero of the destination's type and nothing is loaded: a run wholly behind it loads no plane, the run it cuts loads its
    // live elements one by one.
    const int64_t* live_len;
    int32_t bg_only;                // every destination is the background (a ragged batch's plain download): hi / lo are not loaded
};

// The per-sample arithmetic of an emission, shared by the kernels that write it (emit_body) and that measure it (devio_levels):
// a of sample j1 - 1 of a stream whose tables say at (target) and ac (current), inside a fade of `ramp` samples or behind it
__device__ inline double emit_gain_at(double at, double ac, int64_t j1, int64_t ramp) {
    // (only inside a fade: no call in steady state, ramp == 0, reaches the float64 divide)
    return j1 < ramp ? fma(at - ac, (double)j1 / (double)ramp, ac) : at;
}

// the three float64 signals of one sample: h + l (or h, infinite), the fp32 background widened, x - bg or fma(-ak, bg, x); a
// sample that is not live is zero in all three by a select
// (bf: the background the foreground takes, b itself but for a live handle's shaped foreground)
__device__ inline void emit_sample(float h, float l, float b, float bf, bool live, bool gain, double ak, double& mix, double& bgv, double& fgv) {
    // (an infinite float64 sample narrows to an infinite hi and a NaN remainder: the sample is hi. So it is with a zero
    // remainder, which adds nothing and must not: -0 + +0 is +0, and the mixture of a negative zero is a negative zero)
    const double x = (fabsf(h) <= 3.402823466e38f || h != h) && l != 0.f ? (double)h + (double)l : (double)h;
    mix = live ? x : 0.0;
    const double f = gain ? fma(-ak, (double)bf, x) : x - (double)bf;
    fgv = live ? f : 0.0;
    bgv = live ? (double)b : 0.0;
}

template <typename T, int EPT>
__device__ inline void emit_body(const EmitArgs& a) {
    const int64_t i0 = ((int64_t)blockIdx.x * kIoThreads + threadIdx.x) * EPT;
    if (i0 >= a.count) return;
    const int m = a.count - i0 < EPT ? (int)(a.count - i0) : EPT;
    const int64_t s0 = i0 / a.per, r0 = i0 - s0 * a.per;
    float b[EPT], h[EPT], l[EPT];
    bool live[EPT];
    // rd[k]: element k is read at all (inside the emission and, for a ragged batch, below its clip's length); whole: every
    // element of a full run is, so the vector loads apply
    bool rd[EPT];
    bool whole = m == EPT;
#pragma unroll
    for (int k = 0; k < EPT; ++k) rd[k] = k < m;
    if (a.live_len) {
        // sample and channel of the run's first element (one division, 32-bit where a stream's share allows), then stepped; the
        // length is loaded once and again only where the run enters the next stream
        int64_t s = s0, j;
        int32_t c;
        if (a.per <= 0xffffffffll) {
            const uint32_t q = (uint32_t)r0 / (uint32_t)a.n_channels;
            j = q; c = (int32_t)((uint32_t)r0 - q * (uint32_t)a.n_channels);
        } else {
            j = r0 / a.n_channels; c = (int32_t)(r0 - j * a.n_channels);
        }
        int64_t len = a.live_len[s];
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            if (k < m) {
                rd[k] = j < len;
                whole = whole && rd[k];
                if (++c == a.n_channels) {
                    c = 0;
                    if (++j == a.n_samples) {
                        j = 0; ++s;
                        if (k < m - 1) len = a.live_len[s];
                    }
                }
            }
        }
    }
    if (whole) {
        load_run<EPT>(a.bg + i0, b);
    } else {
#pragma unroll
        for (int k = 0; k < EPT; ++k) b[k] = rd[k] ? a.bg[i0 + k] : 0.f;
    }
    float bf[EPT];
    if (a.bg_fg) {
        if (whole) {
            load_run<EPT>(a.bg_fg + i0, bf);
        } else {
#pragma unroll
            for (int k = 0; k < EPT; ++k) bf[k] = rd[k] ? a.bg_fg[i0 + k] : 0.f;
        }
    } else {
#pragma unroll
        for (int k = 0; k < EPT; ++k) bf[k] = b[k];
    }
    const float* ph = a.hi + s0 * a.in_stream + r0;
    const bool one_stream = whole && r0 + EPT <= a.per;
    if (a.bg_only) {
#pragma unroll
        for (int k = 0; k < EPT; ++k) { h[k] = 0.f; l[k] = 0.f; }
    } else if (one_stream && !(reinterpret_cast<uintptr_t>(ph) & (EPT * 4 - 1))) {
        load_run<EPT>(ph, h);
        if (a.lo) {
            load_run<EPT>(a.lo + s0 * a.in_stream + r0, l);         // (hi and lo are laid out alike: aligned together)
        } else {
#pragma unroll
            for (int k = 0; k < EPT; ++k) l[k] = 0.f;
        }
    } else {
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            h[k] = 0.f; l[k] = 0.f;
            if (rd[k]) {
                int64_t s = s0, r = r0 + k;
                if (r >= a.per) { s += r / a.per; r %= a.per; }
                h[k] = a.hi[s * a.in_stream + r];
                if (a.lo) l[k] = a.lo[s * a.in_stream + r];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        live[k] = a.live_len ? rd[k] : true;
        if (a.slot_start && k < m) {
            int64_t s = s0, r = r0 + k;
            if (r >= a.per) { s += r / a.per; r %= a.per; }
            const int64_t start = a.slot_start[s];
            live[k] = live[k] && start < repet_eng::kSlotIdle && a.pos0 + r / a.n_channels >= start * a.hop;
        }
    }
    double ak[EPT];
    if (a.gain) {
        int64_t s_of = -1;
        double at = (double)a.a, ac = at;
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            ak[k] = at;
            if (a.gain == kGainTables && k < m) {
                int64_t s = s0, r = r0 + k;
                if (r >= a.per) { s += r / a.per; r %= a.per; }
                if (s != s_of) {                                  // (one or two streams per thread: one or two reads per table)
                    at = (double)a.a_tgt[s];
                    ac = a.ramp > 0 ? (double)a.a_cur[s] : at;
                    s_of = s;
                }
                const int64_t j1 = r / a.n_channels + 1;
                ak[k] = emit_gain_at(at, ac, j1, a.ramp);
            }
        }
    }
    double bgv[EPT], fgv[EPT], mix[EPT];
#pragma unroll
    for (int k = 0; k < EPT; ++k) emit_sample(h[k], l[k], b[k], bf[k], live[k], a.gain != 0, a.gain ? ak[k] : 0.0, mix[k], bgv[k], fgv[k]);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        if (d >= a.n_out) break;
        const EmitOut o = a.out[d];
        T* dst = static_cast<T*>(o.p);
        T v[EPT];
#pragma unroll
        for (int k = 0; k < EPT; ++k) v[k] = narrow<T>(o.which == REPET_OUT_BACKGROUND ? bgv[k] : (o.which == REPET_OUT_FOREGROUND ? fgv[k] : mix[k]));
        if (m == EPT && o.dense) {
            store_run<T, EPT>(dst + i0, v);
        } else {
            const IoGeo g{a.count, a.n_samples, a.n_channels, o.s_clip, o.s_sample, o.s_channel};
            Walker w(g, i0);
#pragma unroll
            for (int k = 0; k < EPT; ++k) {
                if (k < m) {
                    dst[w.off] = v[k];
                    if (k < m - 1) w.next(g);
                }
            }
        }
    }
}

__global__ __launch_bounds__(kIoThreads) void devio_emit_f64(EmitArgs a) { emit_body<double, 2>(a); }
__global__ __launch_bounds__(kIoThreads) void devio_emit_f32(EmitArgs a) { emit_body<float, 4>(a); }
__global__ __launch_bounds__(kIoThreads) void devio_emit_i16(EmitArgs a) { emit_body<int16_t, kEpt16>(a); }
__global__ __launch_bounds__(kIoThreads) void devio_emit_f16(EmitArgs a) { emit_body<Half, kEpt16>(a); }
__global__ __launch_bounds__(kIoThreads) void devio_emit_bf16(EmitArgs a) { emit_body<BHalf, kEpt16>(a); }

// Levels of an emission (or of an offline result): per stream s and channel c the REPET_LEVEL_FIELDS float64 values of
// include/repet_hip.h -- sums of squares and largest magnitudes of the three signals emit_sample forms, the live samples and
// those whose mixture is not finite -- reduced in ONE fixed shape, so that every call on the same emission returns the same bits
// (no floating-point atomics anywhere):
//   workgroup (x: chunk of kLevelChunk samples, y: stream) walks its chunk's interleaved elements in tiles of `tile` elements, a
//   multiple of the channel count (and of 4 where that leaves a tile of at most 1024: then every full run is one dwordx4 load per
//   plane, where its addresses are aligned). Thread t owns elements 4t .. 4t+3 of every tile: element i of a tile is channel
//   i % C in every tile, so the thread keeps one accumulator set per element of its run, whatever C is (C = 3 never aligns to a
//   vector: the runs simply start on different channels).
//   Then, four fields at a time: the 1024 accumulators go to LDS in tile order; for each channel every thread folds the entries
//   c + C * (t + 256 m) in order of m, the wave folds its 64 values by __shfl_xor (32, 16, .. 1), lane 0 leaves the wave's value
//   in LDS and one thread per field folds the four waves in wave order.
//   A single chunk writes the record itself; otherwise the workgroup writes partial[s][c][chunk][8] and devio_levels_fold (one
//   wave per stream and channel) folds the chunks: lane (u, f) the u-th eighth of them in index order, then u = 0 .. 7 in order.
// Sums are plain IEEE additions (NaN and inf propagate), peaks fmax (NaN skipped, inf kept, 0 with nothing live); unused
// accumulators hold +0, which changes neither.
constexpr int kLevelSlots = kIoThreads * 4;
struct LevelArgs {
    const float* bg; const float* hi; const float* lo;
    int64_t in_stream, per;
    const int64_t* slot_start; int64_t pos0, hop;
    int32_t n_channels, n_chunks, tile;
    const float* a_cur; const float* a_tgt; int64_t ramp; float a; int32_t gain;
    double* dst; double* partial;
    const float* bg_fg;             // as in EmitArgs
    // as in EmitArgs. The walk of stream s simply ends at its live length, as the walk of a clip of that many samples ends at the
    // clip's end: same tiles, same accumulators, same order -- and devio_levels_fold groups the chunks that hold live samples as it
    // would group that clip's. A ragged clip's record is therefore the one-clip record bit for bit.
    const int64_t* live_len;
};

template <int F> __device__ inline double level_fold(double x, double y) {
    if constexpr (F >= REPET_LEVEL_MIX_PEAK && F <= REPET_LEVEL_FG_PEAK) return fmax(x, y);
    else return x + y;
}

__device__ inline double level_fold_rt(int f, double x, double y) {
    return f >= REPET_LEVEL_MIX_PEAK && f <= REPET_LEVEL_FG_PEAK ? fmax(x, y) : x + y;
}

// fields 4 * G .. 4 * G + 3 of every channel, from the threads' accumulators v[field][element of the run]
template <int G>
__device__ inline void level_regroup(const LevelArgs& a, const double (&v)[4][4], double (*slots)[kLevelSlots], double (*waves)[4][4]) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, C = a.n_channels;
    __syncthreads();                                              // (the previous group's entries have been read)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int k = 0; k < 4; ++k) slots[q][4 * t + k] = v[q][k];
    }
    __syncthreads();
    const int64_t s = blockIdx.y;
    for (int c = 0; c < C; ++c) {
        double r[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = 0.0;
        for (int i = c + C * t; i < a.tile; i += C * kIoThreads) {
            r[0] = level_fold<4 * G + 0>(r[0], slots[0][i]); r[1] = level_fold<4 * G + 1>(r[1], slots[1][i]);
            r[2] = level_fold<4 * G + 2>(r[2], slots[2][i]); r[3] = level_fold<4 * G + 3>(r[3], slots[3][i]);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            r[0] = level_fold<4 * G + 0>(r[0], __shfl_xor(r[0], d)); r[1] = level_fold<4 * G + 1>(r[1], __shfl_xor(r[1], d));
            r[2] = level_fold<4 * G + 2>(r[2], __shfl_xor(r[2], d)); r[3] = level_fold<4 * G + 3>(r[3], __shfl_xor(r[3], d));
        }
        double (*w)[4] = waves[c & 1];                            // (two images: the fold of channel c reads one while c + 1 fills the other)
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) w[wave][q] = r[q];
        }
        __syncthreads();
        if (t < 4) {
            const int f = 4 * G + t;
            double x = w[0][t];
            for (int k = 1; k < kIoThreads / 64; ++k) x = level_fold_rt(f, x, w[k][t]);
            const int64_t sc = s * C + c;
            if (a.n_chunks == 1) a.dst[sc * REPET_LEVEL_FIELDS + f] = x;
            else a.partial[(sc * a.n_chunks + blockIdx.x) * REPET_LEVEL_FIELDS + f] = x;
        }
    }
}

__global__ __launch_bounds__(kIoThreads) void devio_levels(LevelArgs a) {
    __shared__ double slots[4][kLevelSlots];
    __shared__ double waves[2][kIoThreads / 64][4];
    const int t = threadIdx.x, C = a.n_channels;
    const int64_t s = blockIdx.y;
    const int64_t e0 = (int64_t)blockIdx.x * repet_eng::kLevelChunk * C;                    // the chunk's elements of this stream: [e0, e1)
    int64_t e1 = e0 + repet_eng::kLevelChunk * C < a.per ? e0 + repet_eng::kLevelChunk * C : a.per;
    if (a.live_len) {
        const int64_t end = a.live_len[s] * C;
        e1 = e1 < end ? e1 : end;
    }
    // the first live sample of this stream within the emission (emit_body's rule: slot_start and pos0)
    int64_t live_from = 0;
    bool any_live = true;
    if (a.slot_start) {
        const int64_t start = a.slot_start[s];
        any_live = start < repet_eng::kSlotIdle;
        live_from = any_live ? start * a.hop - a.pos0 : 0;
    }
    double at = (double)a.a, ac = at;
    if (a.gain == kGainTables) {
        at = (double)a.a_tgt[s];
        ac = a.ramp > 0 ? (double)a.a_cur[s] : at;
    }
    const float* bg_s = a.bg + s * a.per;
    const float* hi_s = a.hi + s * a.in_stream;
    const float* lo_s = a.lo ? a.lo + s * a.in_stream : nullptr;
    double energy[3][4], peak[3][4];
    unsigned int n_live[4], n_bad[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int q = 0; q < 3; ++q) { energy[q][k] = 0.0; peak[q][k] = 0.0; }
        n_live[k] = 0u; n_bad[k] = 0u;
    }
    if (4 * t < a.tile) {
        for (int64_t base = e0; base < e1; base += a.tile) {
            const int64_t r0 = base + 4 * t;
            if (r0 >= e1) break;
            int m = a.tile - 4 * t < 4 ? a.tile - 4 * t : 4;
            if (e1 - r0 < m) m = (int)(e1 - r0);
            float b[4], h[4], l[4], bf[4];
            const float* pb = bg_s + r0;
            const float* ph = hi_s + r0;
            if (m == 4 && !((reinterpret_cast<uintptr_t>(pb) | reinterpret_cast<uintptr_t>(ph)) & 15)) {
                const float4 vb = *reinterpret_cast<const float4*>(pb);
                const float4 vh = *reinterpret_cast<const float4*>(ph);
                b[0] = vb.x; b[1] = vb.y; b[2] = vb.z; b[3] = vb.w;
                h[0] = vh.x; h[1] = vh.y; h[2] = vh.z; h[3] = vh.w;
                if (lo_s) {                                          // (hi and lo are laid out alike: aligned together)
                    const float4 vl = *reinterpret_cast<const float4*>(lo_s + r0);
                    l[0] = vl.x; l[1] = vl.y; l[2] = vl.z; l[3] = vl.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) l[k] = 0.f;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    b[k] = 0.f; h[k] = 0.f; l[k] = 0.f;
                    if (k < m) {
                        b[k] = pb[k]; h[k] = ph[k];
                        if (lo_s) l[k] = lo_s[r0 + k];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) bf[k] = b[k];
            if (a.bg_fg) {                                        // (laid out like bg: aligned together)
                const float* pf = a.bg_fg + s * a.per + r0;
                if (m == 4 && !(reinterpret_cast<uintptr_t>(pf) & 15)) {
                    const float4 vf = *reinterpret_cast<const float4*>(pf);
                    bf[0] = vf.x; bf[1] = vf.y; bf[2] = vf.z; bf[3] = vf.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) bf[k] = k < m ? pf[k] : 0.f;
                }
            }
            int64_t j = r0 / C;                                   // sample of the run's first element, and its channel
            int c = (int)(r0 - j * C);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool live = k < m && any_live && j >= live_from;
                const double ak = a.gain == kGainTables ? emit_gain_at(at, ac, j + 1, a.ramp) : at;
                double mix, bgv, fgv;
                emit_sample(h[k], l[k], b[k], bf[k], live, a.gain != 0, ak, mix, bgv, fgv);
                energy[0][k] += mix * mix; energy[1][k] += bgv * bgv; energy[2][k] += fgv * fgv;
                peak[0][k] = fmax(peak[0][k], fabs(mix)); peak[1][k] = fmax(peak[1][k], fabs(bgv)); peak[2][k] = fmax(peak[2][k], fabs(fgv));
                n_live[k] += live ? 1u : 0u;
                n_bad[k] += live && !(fabs(mix) <= 1.7976931348623157e308) ? 1u : 0u;
                if (++c == C) { c = 0; ++j; }
            }
        }
    }
    double v[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[0][k] = energy[0][k]; v[1][k] = energy[1][k]; v[2][k] = energy[2][k]; v[3][k] = peak[0][k]; }
    level_regroup<0>(a, v, slots, waves);
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[0][k] = peak[1][k]; v[1][k] = peak[2][k]; v[2][k] = (double)n_live[k]; v[3][k] = (double)n_bad[k]; }
    level_regroup<1>(a, v, slots, waves);
}

// live_len (nullable; C channels per stream): only the chunks that hold live samples of the stream are folded, in the grouping a
// clip of that length has (one chunk: 0 + x, which is x)
__global__ __launch_bounds__(64) void devio_levels_fold(const double* __restrict__ partial, int32_t n_chunks, double* __restrict__ dst,
                                                        const int64_t* __restrict__ live_len, int32_t C) {
    const int f = threadIdx.x & 7, u = threadIdx.x >> 3;
    const int64_t sc = blockIdx.x;
    int n_fold = n_chunks;
    if (live_len) {
        const int64_t used = (live_len[sc / C] + repet_eng::kLevelChunk - 1) / repet_eng::kLevelChunk;
        n_fold = used < n_chunks ? (int)used : n_chunks;
    }
    const int per = (n_fold + 7) / 8;
    const int first = u * per, last = first + per < n_fold ? first + per : n_fold;
    double x = 0.0;
    for (int k = first; k < last; ++k) x = level_fold_rt(f, x, partial[(sc * n_chunks + k) * REPET_LEVEL_FIELDS + f]);
    double r = x;
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        const double y = __shfl(x, 8 * k + f);
        r = level_fold_rt(f, r, y);
    }
    if (u == 0) dst[sc * REPET_LEVEL_FIELDS + f] = r;
}

// simonline over a RAGGED batch (exec_simonline) runs every stage at the frame count T of the pitch. Clip b (blockIdx.y) has
// T_b = repet_frame_count(lengths[b], W, H, 0) frames of its own; the rows [T_b, T) of its spectra are frames the one-clip call
// never forms -- partly the clip's last samples, partly the zero fill, NaN under the reference's 0 / 0 -- and they overlap the
// clip's last hop in the overlap-add. This launch, between the mask stage and the inverse STFT, makes them ZERO in what the
// inverse STFT (plain and shaped) fetches: the spectra X and, where the mask is a plane of its own, Mk -- a store, so that they
// add exactly nothing there (a product with 0 would keep a NaN). blockIdx.z is the channel; the length is one scalar load per
// wave; rows are FS (a multiple of 32) elements, so every store is whole and 16 bytes wide.
__global__ __launch_bounds__(kIoThreads) void devio_tail_clear(float2* __restrict__ X, float* __restrict__ Mk, int64_t spec_stride,
                                                               int64_t chan_stride, int64_t T, int32_t FS, int32_t W, int32_t H,
                                                               const int64_t* __restrict__ lengths) {
    const int64_t num = lengths[blockIdx.y] - W;                  // repet_frame_count(n, W, H, 0)
    int64_t Tb = (num >= 0 ? (num + H - 1) / H : -((-num) / H)) + 1;
    Tb = Tb > 0 ? Tb : 0;
    if (Tb >= T) return;
    const int64_t base = (int64_t)blockIdx.y * spec_stride + (int64_t)blockIdx.z * chan_stride + Tb * FS;
    const int64_t n = (T - Tb) * FS;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t i = ((int64_t)blockIdx.x * kIoThreads + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * kIoThreads * 4) {
        float4* x = reinterpret_cast<float4*>(X + base + i);
        x[0] = zero; x[1] = zero;
        if (Mk) *reinterpret_cast<float4*>(Mk + base + i) = zero;
    }
}

// ---- the streaming handle's per-push data movement (engine_online.hip): S streams at a per-stream stride -------------------
// Grids are streams (y) x four-element slots (x), both capped and walked grid-stride; every store of a whole slot is one
// dwordx4. kRowCopyParts parts (z) per launch. append, feed and take align their slots on the destination offset and walk them
// themselves; every other kernel that moves rows (copies, held slide, slot reset, slot export / import) calls move_part.
constexpr int kMaxIoGroups = 4096;        // workgroups of one launch (16 per CU and more: several rounds of the grid)

// Append: stream b's chunk [n][C] (strided source of any dtype; IoGeo's clip = stream) goes to hi / lo at b * d_stream + d_off,
// as fp32 + fp32 remainder (0 for sources that are not float64). The slots are aligned on the DESTINATION (d_stream % 4 == 0,
// hi / lo 16-byte aligned): the first one of a stream starts d_off % 4 elements before its first sample.
template <typename T>
__device__ inline void append_body(const T* __restrict__ src, IoGeo g, int32_t n_streams, float* __restrict__ hi_out,
                                   float* __restrict__ lo_out, int64_t d_stream, int64_t d_off) {
    const int64_t per = g.n_samples * g.n_channels;
    const int64_t head = d_off & 3;
    const int64_t slots = (head + per + 3) >> 2;
    bool unused = false;
    for (int64_t b = blockIdx.y; b < n_streams; b += gridDim.y) {
        float* hi_b = hi_out + b * d_stream + d_off - head;
        float* lo_b = lo_out + b * d_stream + d_off - head;
        for (int64_t q = (int64_t)blockIdx.x * kIoThreads + threadIdx.x; q < slots; q += (int64_t)gridDim.x * kIoThreads) {
            const int64_t j0 = q * 4 - head;                      // chunk element of the slot's first position
            if (j0 >= 0 && j0 + 4 <= per) {
                float h[4], l[4];
                Walker w(g, b * per + j0);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    split1<T>(src + w.off, h[k], l[k], unused, false);
                    if (k < 3) w.next(g);
                }
                *reinterpret_cast<float4*>(hi_b + q * 4) = make_float4(h[0], h[1], h[2], h[3]);
                *reinterpret_cast<float4*>(lo_b + q * 4) = make_float4(l[0], l[1], l[2], l[3]);
            } else {                                              // first / last slot of a stream: element by element
                for (int k = 0; k < 4; ++k) {
                    const int64_t j = j0 + k;
                    if (j < 0 || j >= per) continue;
                    Walker w(g, b * per + j);
                    float h, l;
                    split1<T>(src + w.off, h, l, unused, false);
                    hi_b[q * 4 + k] = h;
                    lo_b[q * 4 + k] = l;
                }
            }
        }
    }
}

__global__ __launch_bounds__(kIoThreads) void online_append_f64(const double* src, IoGeo g, int32_t s, float* hi, float* lo, int64_t ds, int64_t off) { append_body<double>(src, g, s, hi, lo, ds, off); }
__global__ __launch_bounds__(kIoThreads) void online_append_f32(const float* src, IoGeo g, int32_t s, float* hi, float* lo, int64_t ds, int64_t off) { append_body<float>(src, g, s, hi, lo, ds, off); }
__global__ __launch_bounds__(kIoThreads) void online_append_i16(const int16_t* src, IoGeo g, int32_t s, float* hi, float* lo, int64_t ds, int64_t off) { append_body<int16_t>(src, g, s, hi, lo, ds, off); }
__global__ __launch_bounds__(kIoThreads) void online_append_f16(const Half* src, IoGeo g, int32_t s, float* hi, float* lo, int64_t ds, int64_t off) { append_body<Half>(src, g, s, hi, lo, ds, off); }
__global__ __launch_bounds__(kIoThreads) void online_append_bf16(const BHalf* src, IoGeo g, int32_t s, float* hi, float* lo, int64_t ds, int64_t off) { append_body<BHalf>(src, g, s, hi, lo, ds, off); }

// ---- runs of floats moved in slots of four: the one body of the row copies, the held slide, the slot reset and the slot
// export / import below. A part moves `blocks` runs of `len` floats; slot q of it is four consecutive floats of one run. A whole
// slot is one dwordx4 store where the destination side is aligned (dst_vec) and one dwordx4 load where the source side is
// (src_vec), element accesses otherwise. fill_run (host, below) is the one place that fills a part and decides the two flags; a
// value-initialised part is empty (no slots).
struct RunPart {
    const float* src = nullptr; float* dst = nullptr;
    int64_t len = 0, slots_per_block = 1, blocks = 0, src_block = 0, dst_block = 0;
    int32_t src_vec = 0, dst_vec = 0;
};

// Slot q of part p, between the bases a kernel worked out for its stream or slot: element i of a run is src[blk * src_block + i]
// for i >= zero_below and zero below it -- the source is never read there, so src may point in front of what the source holds.
// Nothing is stored at or behind `len` (a kernel may cut the part's own). load4: a whole slot may be loaded as one dwordx4.
__device__ inline void move_slot(const RunPart& p, int64_t q, const float* src, float* dst, int64_t len, int64_t zero_below, bool load4) {
    const int64_t blk = q / p.slots_per_block;
    const int64_t i0 = (q - blk * p.slots_per_block) * 4;
    if (i0 >= len) return;
    float* d = dst + blk * p.dst_block + i0;
    const int64_t so = blk * p.src_block + i0;
    if (i0 + 4 <= len && p.dst_vec) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i0 >= zero_below) {
            if (load4) v = *reinterpret_cast<const float4*>(src + so);
            else v = make_float4(src[so], src[so + 1], src[so + 2], src[so + 3]);
        } else if (i0 + 4 > zero_below) {                         // the slot the boundary cuts
            float e[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) e[k] = i0 + k >= zero_below ? src[so + k] : 0.f;
            v = make_float4(e[0], e[1], e[2], e[3]);
        }
        *reinterpret_cast<float4*>(d) = v;
    } else {
        const int64_t m = len - i0 < 4 ? len - i0 : 4;
        for (int64_t k = 0; k < m; ++k) d[k] = i0 + k >= zero_below ? src[so + k] : 0.f;
    }
}

// the workgroups of grid x walk the part's slots grid-stride. A null source is the boundary at len: the part stores zeros.
__device__ inline void move_part(const RunPart& p, const float* src, float* dst, int64_t len, int64_t zero_below, bool load4) {
    const int64_t slots = p.slots_per_block * p.blocks;
    if (!src) zero_below = len;
    for (int64_t q = (int64_t)blockIdx.x * kIoThreads + threadIdx.x; q < slots; q += (int64_t)gridDim.x * kIoThreads)
        move_slot(p, q, src, dst, len, zero_below, load4);
}

// Row copies: part z moves its runs for every stream (or writes zeros where src is null), stream b at b * src_stream /
// b * dst_stream floats. A part with row_len > 0 covers frame rows: see engine.h.
struct RowCopyDev { RunPart run; int64_t src_stream, dst_stream, row_len, frame0; };
struct RowCopyArgs { RowCopyDev part[repet_eng::kRowCopyParts]; int32_t n_streams; const int64_t* slot_start; };

__global__ __launch_bounds__(kIoThreads) void online_row_copies(RowCopyArgs a) {
    const RowCopyDev& p = a.part[blockIdx.z];
    for (int64_t b = blockIdx.y; b < a.n_streams; b += gridDim.y) {
        int64_t len = p.run.len;
        if (p.row_len > 0) {                                      // only the frame rows before the slot's own first frame
            const int64_t rows = a.slot_start ? a.slot_start[b] - p.frame0 : 0;
            len = rows <= 0 ? 0 : (rows < p.run.len / p.row_len ? rows * p.row_len : p.run.len);
        }
        move_part(p.run, p.run.src ? p.run.src + b * p.src_stream : nullptr, p.run.dst + b * p.dst_stream, len, 0, p.run.src_vec != 0);
    }
}

// The slide of a push during which slots are HELD (repet_online_hold_streams): the row copies above, except that a stream whose
// table entry is kSlotHeld takes element i of a run from `held_delta` floats further on in its source (<= 0: its content stays
// where it is while the others' moves down) for i >= zero_below, and zero below it -- the offset may point in front of the
// stream's share (the runs in front of a held slot's content while the handle's history grows). held_vec: src_vec of the
// shifted source.
struct SlideDev { RunPart run; int64_t src_stream, dst_stream, held_delta, zero_below; int32_t held_vec; };
struct SlideArgs { SlideDev part[repet_eng::kRowCopyParts]; int32_t n_streams; const int64_t* slot_start; };

__global__ __launch_bounds__(kIoThreads) void online_slide_held(SlideArgs a) {
    const SlideDev& p = a.part[blockIdx.z];
    for (int64_t b = blockIdx.y; b < a.n_streams; b += gridDim.y) {
        const bool held = a.slot_start[b] == repet_eng::kSlotHeld;
        move_part(p.run, p.run.src + b * p.src_stream + (held ? p.held_delta : 0), p.run.dst + b * p.dst_stream, p.run.len,
                  held ? p.zero_below : 0, held ? p.held_vec != 0 : p.run.src_vec != 0);
    }
}

// Hold / resume: table[slot[i]] = value[i] (kSlotHeld, or the slot's own first frame again). One workgroup.
struct SlotSetArgs { int64_t* table; int32_t n; unsigned short slot[repet_eng::kSlotResetIds]; int64_t value[repet_eng::kSlotResetIds]; };
__global__ __launch_bounds__(kIoThreads) void online_slot_set(SlotSetArgs g) {
    for (int32_t i = threadIdx.x; i < g.n; i += kIoThreads) g.table[g.slot[i]] = g.value[i];
}

// ---- per-slot inboxes (repet_online_enable_feed): slot b owns a ring of ring_len = capacity * C floats per plane (hi, and lo
// for the fp32 remainders of float64 sources) at b * ring_stride; queued sample p of it lies at float (p * C) % ring_len. The
// host mirrors every read and write position and hands them over in the kernel arguments (the SlotSetArgs pattern: no copy
// to the device and no wait); both kernels wrap inside. Slots of four floats aligned on the side that is stored to, as above.
//
// Feed: row r of the source [rows][n][C] (strided, any ingest dtype; IoGeo's clip = row) brings its first count[r] samples to
// the ring of slot[r], from float wpos[r] on. What lies behind count[r] in a row is never read. The conversions are append's.
struct FeedArgs {
    float* hi; float* lo; int64_t ring_stride, ring_len; int32_t row0, n_rows;
    unsigned short slot[repet_eng::kSlotResetIds]; int32_t count[repet_eng::kSlotResetIds]; int32_t wpos[repet_eng::kSlotResetIds];
};

template <typename T>
__device__ inline void feed_body(const T* __restrict__ src, IoGeo g, const FeedArgs& a) {
    const int64_t per = g.n_samples * g.n_channels;
    bool unused = false;
    for (int32_t r = blockIdx.y; r < a.n_rows; r += gridDim.y) {
        const int64_t len = (int64_t)a.count[r] * g.n_channels, w0 = a.wpos[r], head = w0 & 3;
        const int64_t slots = (head + len + 3) >> 2, row = (int64_t)(a.row0 + r) * per;
        float* hi_b = a.hi + a.slot[r] * a.ring_stride;
        float* lo_b = a.lo + a.slot[r] * a.ring_stride;
        for (int64_t q = (int64_t)blockIdx.x * kIoThreads + threadIdx.x; q < slots; q += (int64_t)gridDim.x * kIoThreads) {
            const int64_t j0 = q * 4 - head;                      // row element of the slot's first position
            int64_t d0 = w0 + j0;
            if (d0 >= a.ring_len) d0 -= a.ring_len;
            if (j0 >= 0 && j0 + 4 <= len && d0 + 4 <= a.ring_len && !(d0 & 3)) {
                float h[4], l[4];
                Walker w(g, row + j0);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    split1<T>(src + w.off, h[k], l[k], unused, false);
                    if (k < 3) w.next(g);
                }
                *reinterpret_cast<float4*>(hi_b + d0) = make_float4(h[0], h[1], h[2], h[3]);
                *reinterpret_cast<float4*>(lo_b + d0) = make_float4(l[0], l[1], l[2], l[3]);
            } else {                                              // first / last slot of a row, and the one the wrap cuts
                for (int k = 0; k < 4; ++k) {
                    const int64_t j = j0 + k;
                    if (j < 0 || j >= len) continue;
                    int64_t d = w0 + j;
                    if (d >= a.ring_len) d -= a.ring_len;
                    Walker w(g, row + j);
                    float h, l;
                    split1<T>(src + w.off, h, l, unused, false);
                    hi_b[d] = h;
                    lo_b[d] = l;
                }
            }
        }
    }
}

__global__ __launch_bounds__(kIoThreads) void online_feed_f64(const double* src, IoGeo g, FeedArgs a) { feed_body<double>(src, g, a); }
__global__ __launch_bounds__(kIoThreads) void online_feed_f32(const float* src, IoGeo g, FeedArgs a) { feed_body<float>(src, g, a); }
__global__ __launch_bounds__(kIoThreads) void online_feed_i16(const int16_t* src, IoGeo g, FeedArgs a) { feed_body<int16_t>(src, g, a); }
__global__ __launch_bounds__(kIoThreads) void online_feed_f16(const Half* src, IoGeo g, FeedArgs a) { feed_body<Half>(src, g, a); }
__global__ __launch_bounds__(kIoThreads) void online_feed_bf16(const BHalf* src, IoGeo g, FeedArgs a) { feed_body<BHalf>(src, g, a); }

// Take (the append of a tick): `len` floats of both planes from float rpos[i] of slot first + i's ring go to its share of the
// pending buffers at dst_off, where online_append_* would have written them. A slot whose table entry is idle or held -- the
// caller's holds and the starved slots of this tick -- is skipped: nothing of its ring is read and nothing of its share written.
struct TakeArgs {
    const float* hi; const float* lo; int64_t ring_stride, ring_len; float* dst_hi; float* dst_lo; int64_t dst_stream, dst_off, len;
    const int64_t* slot_start; int32_t first, n_slots; int32_t rpos[repet_eng::kSlotResetIds];
};

__device__ inline void take4(const float* __restrict__ ring, int64_t s0, int64_t ring_len, float (&v)[4]) {
    if (s0 + 4 <= ring_len) {
        if (!(s0 & 3)) {
            const float4 x = *reinterpret_cast<const float4*>(ring + s0);
            v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = ring[s0 + k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = ring[s0 + k < ring_len ? s0 + k : s0 + k - ring_len];
    }
}

__global__ __launch_bounds__(kIoThreads) void online_take(TakeArgs a) {
    const int64_t head = a.dst_off & 3;
    const int64_t slots = (head + a.len + 3) >> 2;
    for (int32_t i = blockIdx.y; i < a.n_slots; i += gridDim.y) {
        const int64_t b = a.first + i;
        if (a.slot_start[b] >= repet_eng::kSlotIdle) continue;
        const float* sh = a.hi + b * a.ring_stride;
        const float* sl = a.lo + b * a.ring_stride;
        float* dh = a.dst_hi + b * a.dst_stream + a.dst_off - head;
        float* dl = a.dst_lo + b * a.dst_stream + a.dst_off - head;
        const int64_t r0 = a.rpos[i];
        for (int64_t q = (int64_t)blockIdx.x * kIoThreads + threadIdx.x; q < slots; q += (int64_t)gridDim.x * kIoThreads) {
            const int64_t j0 = q * 4 - head;
            if (j0 >= 0 && j0 + 4 <= a.len) {
                int64_t s0 = r0 + j0;
                if (s0 >= a.ring_len) s0 -= a.ring_len;
                float h[4], l[4];
                take4(sh, s0, a.ring_len, h);
                take4(sl, s0, a.ring_len, l);
                *reinterpret_cast<float4*>(dh + q * 4) = make_float4(h[0], h[1], h[2], h[3]);
                *reinterpret_cast<float4*>(dl + q * 4) = make_float4(l[0], l[1], l[2], l[3]);
            } else {
                for (int k = 0; k < 4; ++k) {
                    const int64_t j = j0 + k;
                    if (j < 0 || j >= a.len) continue;
                    int64_t s = r0 + j;
                    if (s >= a.ring_len) s -= a.ring_len;
                    dh[q * 4 + k] = sh[s];
                    dl[q * 4 + k] = sl[s];
                }
            }
        }
    }
}

// Slot reset (restart / release of slots of the streaming handle): workgroups (x, slot of the list, part) write the part's
// runs of zeros (no part has a source) into that slot's share of the buffers, and one thread per slot its new first frame.
struct ZeroPartDev { RunPart run; int64_t dst_stream; };
struct SlotResetArgs {
    ZeroPartDev part[repet_eng::kRowCopyParts]; int64_t* slot_start; int64_t value; int32_t n_slots;
    unsigned short slot[repet_eng::kSlotResetIds];
};

__global__ __launch_bounds__(kIoThreads) void online_slot_reset(SlotResetArgs a) {
    const int64_t b = a.slot[blockIdx.y];
    if (blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x == 0) a.slot_start[b] = a.value;
    const ZeroPartDev& p = a.part[blockIdx.z];
    move_part(p.run, nullptr, p.run.dst + b * p.dst_stream, p.run.len, 0, false);
}

// Slot export / import (a live stream moved between handles): part y moves its runs between ONE slot's share of the handle's
// strided buffers and the dense payload. Element i of a run is src[src_off + blk * src_block + i] for i >= zero_below and zero
// below it (src_off may be negative, the run right-aligned on what the source holds). The import also writes the slot's first
// frame and, where the handle's epoch moved with it, adds `shift` to the first frame of every other live slot (one workgroup,
// plain stores).
struct SlotMoveDev { RunPart run; int64_t src_off, zero_below; };
struct SlotMoveArgs { SlotMoveDev part[repet_eng::kRowCopyParts]; int64_t* slot_start; int64_t value, shift; int32_t slot, n_slots; };

__device__ inline void slot_move_body(const SlotMoveDev& p) {
    move_part(p.run, p.run.src ? p.run.src + p.src_off : nullptr, p.run.dst, p.run.len, p.zero_below, p.run.src_vec != 0);
}

__global__ __launch_bounds__(kIoThreads) void online_slot_export(SlotMoveArgs a) { slot_move_body(a.part[blockIdx.y]); }

__global__ __launch_bounds__(kIoThreads) void online_slot_import(SlotMoveArgs a) {
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        for (int32_t s = threadIdx.x; s < a.n_slots; s += kIoThreads) {
            if (s == a.slot) a.slot_start[s] = a.value;
            else if (a.shift != 0 && a.slot_start[s] < repet_eng::kSlotIdle) a.slot_start[s] += a.shift;
        }
    }
    slot_move_body(a.part[blockIdx.y]);
}

// Background gains of the streaming handle: fp32 tables [S] of a = (float)(1 - gain). One workgroup each.
__global__ __launch_bounds__(kIoThreads) void online_gain_fill(float* table, int32_t n, float a) {
    for (int32_t i = threadIdx.x; i < n; i += kIoThreads) table[i] = a;
}

struct GainSetArgs { float* tgt; int32_t n; unsigned short slot[repet_eng::kSlotResetIds]; float a[repet_eng::kSlotResetIds]; };
__global__ __launch_bounds__(kIoThreads) void online_gain_set(GainSetArgs g) {
    for (int32_t i = threadIdx.x; i < g.n; i += kIoThreads) g.tgt[g.slot[i]] = g.a[i];
}

__global__ __launch_bounds__(kIoThreads) void online_gain_commit(const float* tgt, const float* cur_old, float* cur_new, int32_t n, int32_t slot) {
    for (int32_t i = threadIdx.x; i < n; i += kIoThreads) cur_new[i] = slot < 0 || i == slot ? tgt[i] : cur_old[i];
}

// Band gains of the streaming handle (engine.h: bands). expand: workgroup (x, named slot i) writes bins of the slot's pending
// row; the band of a bin by bisection over the ascending edges (up to F + 1 of them). Everything it reads of the job lies
// inside band_job_words() words; everything it writes inside the slot's three rows.
struct BandExpandArgs { float* tab; const int32_t* job; int32_t FS, F, n, n_bands, rows, init; };
__global__ __launch_bounds__(kIoThreads) void online_band_expand(BandExpandArgs a) {
    const int32_t i = blockIdx.y;
    const int32_t* slot = a.job;
    const int32_t* row = slot + a.n;
    const int32_t* edges = row + a.n;
    const float* gains = reinterpret_cast<const float*>(edges + a.n_bands + 1);
    const int32_t r = row[i];
    float* base = a.tab + (int64_t)slot[i] * repet_eng::kBandRows * a.FS;
    for (int32_t k = blockIdx.x * kIoThreads + threadIdx.x; k < a.FS; k += gridDim.x * kIoThreads) {
        float g = 0.f;
        if (r >= 0 && r < a.rows && k < a.F && k >= edges[0] && k < edges[a.n_bands]) {
            int32_t lo = 0, hi = a.n_bands;                       // edges[lo] <= k < edges[hi]
            while (hi - lo > 1) {
                const int32_t mid = (lo + hi) >> 1;
                if (edges[mid] <= k) lo = mid; else hi = mid;
            }
            g = gains[(int64_t)r * a.n_bands + lo];
        }
        base[repet_eng::kBandPending * a.FS + k] = (float)(1.0 - (double)g);
        if (a.init) { base[repet_eng::kBandCarried * a.FS + k] = 1.f; base[repet_eng::kBandNew * a.FS + k] = 1.f; }
    }
}

// commit / settle: workgroup (x, slot). A thread moves its own bins only, so the rows of a slot need no order between threads.
__global__ __launch_bounds__(kIoThreads) void online_band_commit(float* tab, int32_t FS, int32_t slot, int32_t mode, const int64_t* slot_start) {
    const int32_t s = slot < 0 ? (int32_t)blockIdx.y : slot;
    if (slot < 0 && slot_start && slot_start[s] == repet_eng::kSlotHeld) return;
    float* base = tab + (int64_t)s * repet_eng::kBandRows * FS;
    for (int32_t k = blockIdx.x * kIoThreads + threadIdx.x; k < FS; k += gridDim.x * kIoThreads) {
        const float p = base[repet_eng::kBandPending * FS + k], n = base[repet_eng::kBandNew * FS + k];
        base[repet_eng::kBandCarried * FS + k] = mode == repet_eng::kBandSettle ? p : n;
        if (mode != repet_eng::kBandCarry) base[repet_eng::kBandNew * FS + k] = p;
    }
}

int element_size(int dtype) {
    switch (dtype) {
        case REPET_F64: return 8;
        case REPET_F32: return 4;
        case REPET_I16: case REPET_F16: case REPET_BF16: return 2;
        default: return 0;                                        // not a dtype
    }
}

// the strided side is the interleaved layout itself (strides of a C-contiguous [clip][n][c]; a size-1 dimension's stride
// does not matter) and its base allows a vector access of `vec_bytes`
bool is_dense(const void* p, const IoGeo& g, int32_t n_clips, int vec_bytes) {
    if (reinterpret_cast<uintptr_t>(p) % vec_bytes) return false;
    if (g.n_channels > 1 && g.s_channel != 1) return false;
    if (g.n_samples > 1 && g.s_sample != g.n_channels) return false;
    if (n_clips > 1 && g.s_clip != g.n_samples * g.n_channels) return false;
    return true;
}

}  // namespace
}  // namespace repet

using namespace repet_eng;
using namespace repet;

namespace repet_eng {

thread_local DevioReport* devio_report = nullptr;

// the grid of a launch, on its way into the <<< >>> (engine.h: DevioReport)
static dim3 noted(dim3 grid) {
    if (devio_report) {
        ++devio_report->launches;
        devio_report->grid[0] = grid.x; devio_report->grid[1] = grid.y; devio_report->grid[2] = grid.z;
    }
    return grid;
}
static int noted_dense(int k, bool dense) {
    if (devio_report) devio_report->dense[k] = dense ? 1 : 0;
    return dense ? 1 : 0;
}
// part k as the kernel will take it (held_vec < 0: the launcher has none)
static void noted_part(int k, const RunPart& r, int held_vec = -1) {
    if (!devio_report) return;
    devio_report->src_vec[k] = r.src_vec; devio_report->dst_vec[k] = r.dst_vec; devio_report->held_vec[k] = held_vec;
}

static dim3 stream_grid(int64_t slots, int32_t n_streams, int parts) {
    const int64_t y = std::min<int64_t>(n_streams, 65535);
    const int64_t x_cap = std::max<int64_t>(1, kMaxIoGroups / (y * parts));
    return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(slots, kIoThreads), x_cap)), (unsigned)y, (unsigned)parts);
}

// one side of a part takes dwordx4 accesses: a 16-byte base, and every stride and offset it is reached through a multiple of four
static bool vec_side(const float* base, int64_t block, int64_t stream) {
    return !(reinterpret_cast<uintptr_t>(base) & 15) && !(block & 3) && !(stream & 3);
}

// fills the part move_part walks and returns its slots, for the grid (0, and the part left empty, where there is nothing to move)
static int64_t fill_run(RunPart& r, const float* src, float* dst, int64_t len, int64_t blocks, int64_t src_block, int64_t dst_block,
                        int64_t src_stream = 0, int64_t dst_stream = 0) {
    r = RunPart{};
    if (len <= 0 || blocks <= 0) return 0;
    r.src = src; r.dst = dst; r.len = len; r.slots_per_block = ceil_div(len, 4); r.blocks = blocks;
    r.src_block = src_block; r.dst_block = dst_block;
    r.dst_vec = vec_side(dst, dst_block, dst_stream) ? 1 : 0;
    r.src_vec = src && vec_side(src, src_block, src_stream) ? 1 : 0;
    return r.slots_per_block * blocks;
}

hipError_t launch_stream_append(const void* src, int dtype, int32_t n_streams, int64_t n, int32_t ch, const int64_t src_strides[3],
                                float* hi, float* lo, int64_t dst_stream, int64_t dst_off, hipStream_t s) {
    if (n <= 0 || n_streams <= 0) return hipSuccess;
    if ((dst_stream & 3) || (reinterpret_cast<uintptr_t>(hi) & 15) || (reinterpret_cast<uintptr_t>(lo) & 15)) return hipErrorInvalidValue;
    IoGeo g{n * ch * n_streams, n, ch, src_strides[0], src_strides[1], src_strides[2]};
    const dim3 grid = stream_grid(ceil_div((dst_off & 3) + n * ch, 4), n_streams, 1);
    switch (dtype) {
        case REPET_F64: online_append_f64<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const double*>(src), g, n_streams, hi, lo, dst_stream, dst_off); break;
        case REPET_F32: online_append_f32<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const float*>(src), g, n_streams, hi, lo, dst_stream, dst_off); break;
        case REPET_I16: online_append_i16<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const int16_t*>(src), g, n_streams, hi, lo, dst_stream, dst_off); break;
        case REPET_F16: online_append_f16<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const Half*>(src), g, n_streams, hi, lo, dst_stream, dst_off); break;
        default: online_append_bf16<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const BHalf*>(src), g, n_streams, hi, lo, dst_stream, dst_off); break;
    }
    return hipGetLastError();
}

hipError_t launch_row_copies(const RowCopy* parts, int n_parts, int32_t n_streams, hipStream_t s, const int64_t* slot_start) {
    if (n_parts <= 0 || n_parts > kRowCopyParts || n_streams <= 0) return n_parts == 0 ? hipSuccess : hipErrorInvalidValue;
    RowCopyArgs a{};
    a.n_streams = n_streams;
    a.slot_start = slot_start;
    int64_t most = 1;
    for (int k = 0; k < n_parts; ++k) {
        const RowCopy& p = parts[k];
        RowCopyDev& d = a.part[k];
        most = std::max(most, fill_run(d.run, p.src, p.dst, p.len, p.blocks, p.src_block, p.dst_block, p.src_stream, p.dst_stream));
        d.src_stream = p.src_stream; d.dst_stream = p.dst_stream; d.row_len = p.row_len; d.frame0 = p.frame0;
        noted_part(k, d.run);
    }
    online_row_copies<<<noted(stream_grid(most, n_streams, n_parts)), kIoThreads, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_slide_held(const RowCopy* parts, const HeldShift* shifts, int n_parts, int32_t n_streams, hipStream_t s,
                             const int64_t* slot_start) {
    if (n_parts <= 0 || n_parts > kRowCopyParts || n_streams <= 0 || !slot_start || !shifts) return hipErrorInvalidValue;
    SlideArgs a{};
    a.n_streams = n_streams;
    a.slot_start = slot_start;
    int64_t most = 1;
    for (int k = 0; k < n_parts; ++k) {
        const RowCopy& p = parts[k];
        const HeldShift& h = shifts[k];
        if (p.len <= 0 || p.blocks <= 0) continue;                // an empty part: no slots
        if (!p.src || !p.dst || p.row_len != 0 || h.delta > 0 || h.zero_below < 0) return hipErrorInvalidValue;
        SlideDev& d = a.part[k];
        most = std::max(most, fill_run(d.run, p.src, p.dst, p.len, p.blocks, p.src_block, p.dst_block, p.src_stream, p.dst_stream));
        d.src_stream = p.src_stream; d.dst_stream = p.dst_stream;
        d.held_delta = h.delta; d.zero_below = std::min(h.zero_below, p.len);
        d.held_vec = d.run.src_vec && !(h.delta & 3) ? 1 : 0;
        noted_part(k, d.run, d.held_vec);
    }
    online_slide_held<<<noted(stream_grid(most, n_streams, n_parts)), kIoThreads, 0, s>>>(a);
    return hipGetLastError();
}

// (the slots of one call are distinct: two threads never write one entry)
hipError_t launch_slot_set(int64_t* slot_start, const int32_t* slots, const int64_t* values, int32_t n_slots, hipStream_t s) {
    if (n_slots <= 0) return hipSuccess;
    if (!slot_start || !slots || !values) return hipErrorInvalidValue;
    SlotSetArgs g{};
    g.table = slot_start;
    for (int32_t first = 0; first < n_slots; first += kSlotResetIds) {
        g.n = std::min<int32_t>(kSlotResetIds, n_slots - first);
        for (int32_t k = 0; k < g.n; ++k) { g.slot[k] = (unsigned short)slots[first + k]; g.value[k] = values[first + k]; }
        online_slot_set<<<noted(dim3(1)), kIoThreads, 0, s>>>(g);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// (the rows of one call name distinct slots and every run fits its ring: two threads never write one float)
hipError_t launch_feed(const void* src, int dtype, int64_t n, int32_t ch, const int64_t src_strides[3], const int32_t* slots,
                       const int64_t* counts, const int64_t* wpos, int32_t n_rows, float* hi, float* lo, int64_t ring_stride,
                       int64_t ring_len, hipStream_t s) {
    if (n_rows <= 0 || n <= 0) return hipSuccess;
    if (!src || !slots || !counts || !wpos || !hi || !lo || ring_len <= 0 || ring_len > INT32_MAX || ring_stride < ring_len ||
        (ring_stride & 3) || (reinterpret_cast<uintptr_t>(hi) & 15) || (reinterpret_cast<uintptr_t>(lo) & 15))
        return hipErrorInvalidValue;
    const IoGeo g{n * ch * n_rows, n, ch, src_strides[0], src_strides[1], src_strides[2]};
    FeedArgs a{};
    a.hi = hi; a.lo = lo; a.ring_stride = ring_stride; a.ring_len = ring_len;
    for (int32_t first = 0; first < n_rows; first += kSlotResetIds) {
        a.row0 = first;
        a.n_rows = std::min<int32_t>(kSlotResetIds, n_rows - first);
        int64_t most = 0;
        for (int32_t k = 0; k < a.n_rows; ++k) {
            const int64_t cnt = counts[first + k], w = wpos[first + k];
            if (cnt < 0 || cnt > n || cnt * ch > ring_len || w < 0 || w >= ring_len || slots[first + k] < 0 || slots[first + k] > 65535)
                return hipErrorInvalidValue;
            a.slot[k] = (unsigned short)slots[first + k]; a.count[k] = (int32_t)cnt; a.wpos[k] = (int32_t)w;
            most = std::max(most, cnt);
        }
        if (most == 0) continue;
        const dim3 grid = stream_grid(ceil_div(3 + most * ch, 4), a.n_rows, 1);
        switch (dtype) {
            case REPET_F64: online_feed_f64<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const double*>(src), g, a); break;
            case REPET_F32: online_feed_f32<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const float*>(src), g, a); break;
            case REPET_I16: online_feed_i16<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const int16_t*>(src), g, a); break;
            case REPET_F16: online_feed_f16<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const Half*>(src), g, a); break;
            case REPET_BF16: online_feed_bf16<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const BHalf*>(src), g, a); break;
            default: return hipErrorInvalidValue;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_take(const float* hi, const float* lo, int64_t ring_stride, int64_t ring_len, const int64_t* rpos, int32_t n_slots,
                       int64_t len, float* dst_hi, float* dst_lo, int64_t dst_stream, int64_t dst_off, const int64_t* slot_start,
                       hipStream_t s) {
    if (n_slots <= 0 || len <= 0) return hipSuccess;
    if (!hi || !lo || !rpos || !dst_hi || !dst_lo || !slot_start || ring_len <= 0 || ring_len > INT32_MAX || len > ring_len ||
        ring_stride < ring_len || (ring_stride & 3) || (dst_stream & 3) || dst_off < 0 || dst_off + len > dst_stream ||
        (reinterpret_cast<uintptr_t>(hi) & 15) || (reinterpret_cast<uintptr_t>(lo) & 15) || (reinterpret_cast<uintptr_t>(dst_hi) & 15) ||
        (reinterpret_cast<uintptr_t>(dst_lo) & 15))
        return hipErrorInvalidValue;
    TakeArgs a{};
    a.hi = hi; a.lo = lo; a.ring_stride = ring_stride; a.ring_len = ring_len; a.dst_hi = dst_hi; a.dst_lo = dst_lo;
    a.dst_stream = dst_stream; a.dst_off = dst_off; a.len = len; a.slot_start = slot_start;
    for (int32_t first = 0; first < n_slots; first += kSlotResetIds) {
        a.first = first;
        a.n_slots = std::min<int32_t>(kSlotResetIds, n_slots - first);
        for (int32_t k = 0; k < a.n_slots; ++k) {
            if (rpos[first + k] < 0 || rpos[first + k] >= ring_len) return hipErrorInvalidValue;
            a.rpos[k] = (int32_t)rpos[first + k];
        }
        online_take<<<noted(stream_grid(ceil_div((dst_off & 3) + len, 4), a.n_slots, 1)), kIoThreads, 0, s>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_slot_reset(int64_t* slot_start, int64_t value, const int32_t* slots, int32_t n_slots, const ZeroPart* parts,
                             int n_parts, hipStream_t s) {
    if (n_slots <= 0) return hipSuccess;
    if (!slot_start || !slots || n_parts < 0 || n_parts > kRowCopyParts) return hipErrorInvalidValue;
    SlotResetArgs a{};
    a.slot_start = slot_start; a.value = value;
    int64_t most = 1;
    for (int k = 0; k < n_parts; ++k) {
        const ZeroPart& p = parts[k];
        most = std::max(most, fill_run(a.part[k].run, nullptr, p.dst, p.len, p.blocks, 0, p.dst_block, 0, p.dst_stream));
        a.part[k].dst_stream = p.dst_stream;
        noted_part(k, a.part[k].run);
    }
    for (int32_t first = 0; first < n_slots; first += kSlotResetIds) {
        a.n_slots = std::min<int32_t>(kSlotResetIds, n_slots - first);
        for (int32_t k = 0; k < a.n_slots; ++k) a.slot[k] = (unsigned short)slots[first + k];
        online_slot_reset<<<noted(stream_grid(most, a.n_slots, kRowCopyParts)), kIoThreads, 0, s>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// the parts of a slot move as the kernels take them; returns the slots of the longest part (-1: a part the kernels cannot take)
static int64_t slot_move_args(const SlotMove* parts, int n_parts, SlotMoveArgs& a) {
    int64_t most = 1;
    for (int k = 0; k < n_parts; ++k) {
        const SlotMove& p = parts[k];
        if (p.len <= 0 || p.blocks <= 0) continue;
        const bool reads = p.src && p.zero_below < p.len;
        if (!p.dst || p.zero_below < 0 || (!p.src && p.zero_below < p.len) || (reads && p.src_off + p.zero_below < 0)) return -1;
        SlotMoveDev& d = a.part[k];
        most = std::max(most, fill_run(d.run, p.src, p.dst, p.len, p.blocks, p.src_block, p.dst_block));
        d.src_off = p.src_off; d.zero_below = std::min(p.zero_below, p.len);
        d.run.src_vec = d.run.src_vec && reads && !(p.src_off & 3) ? 1 : 0;
        noted_part(k, d.run);
    }
    return most;
}

static dim3 slot_move_grid(int64_t most) {
    return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(most, kIoThreads), kMaxIoGroups / kRowCopyParts)), kRowCopyParts);
}

hipError_t launch_slot_export(const SlotMove* parts, int n_parts, hipStream_t s) {
    if (n_parts <= 0 || n_parts > kRowCopyParts) return hipErrorInvalidValue;
    SlotMoveArgs a{};
    const int64_t most = slot_move_args(parts, n_parts, a);
    if (most < 0) return hipErrorInvalidValue;
    online_slot_export<<<noted(slot_move_grid(most)), kIoThreads, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_slot_import(const SlotMove* parts, int n_parts, int64_t* slot_start, int32_t n_slots, int32_t slot, int64_t value,
                              int64_t shift, hipStream_t s) {
    if (n_parts < 0 || n_parts > kRowCopyParts || !slot_start || slot < 0 || slot >= n_slots) return hipErrorInvalidValue;
    SlotMoveArgs a{};
    const int64_t most = slot_move_args(parts, n_parts, a);
    if (most < 0) return hipErrorInvalidValue;
    a.slot_start = slot_start; a.value = value; a.shift = shift; a.slot = slot; a.n_slots = n_slots;
    online_slot_import<<<noted(slot_move_grid(most)), kIoThreads, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_stream_egress(const float* in, int32_t n_streams, int64_t n, int32_t ch, void* dst, int dtype,
                                const int64_t strides[3], hipStream_t s) {
    const int64_t count = (int64_t)n_streams * n * ch;
    if (count <= 0) return hipSuccess;
    IoGeo g{count, n, ch, strides[0], strides[1], strides[2]};
    if (dtype == REPET_F64) {
        const dim3 grid((unsigned)ceil_div(ceil_div(count, 2), kIoThreads));
        devio_egress_f64<<<noted(grid), kIoThreads, 0, s>>>(in, g, noted_dense(0, is_dense(dst, g, n_streams, 16)), static_cast<double*>(dst));
    } else if (dtype == REPET_F32) {
        const dim3 grid((unsigned)ceil_div(ceil_div(count, 4), kIoThreads));
        devio_egress_f32<<<noted(grid), kIoThreads, 0, s>>>(in, g, noted_dense(0, is_dense(dst, g, n_streams, 16)), static_cast<float*>(dst));
    } else {
        // a dense 16-bit destination takes one store of kEpt16 elements per lane: aligned for that, or element by element
        const dim3 grid((unsigned)ceil_div(ceil_div(count, kEpt16), kIoThreads));
        const int dense = noted_dense(0, is_dense(dst, g, n_streams, 2 * kEpt16));
        switch (dtype) {
            case REPET_I16: devio_egress_i16<<<noted(grid), kIoThreads, 0, s>>>(in, g, dense, static_cast<int16_t*>(dst)); break;
            case REPET_F16: devio_egress_f16<<<noted(grid), kIoThreads, 0, s>>>(in, g, dense, static_cast<Half*>(dst)); break;
            case REPET_BF16: devio_egress_bf16<<<noted(grid), kIoThreads, 0, s>>>(in, g, dense, static_cast<BHalf*>(dst)); break;
            default: return hipErrorInvalidValue;
        }
    }
    return hipGetLastError();
}

hipError_t launch_gain_fill(float* table, int32_t n, float a, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!table) return hipErrorInvalidValue;
    online_gain_fill<<<noted(dim3(1)), kIoThreads, 0, s>>>(table, n, a);
    return hipGetLastError();
}

// (the slots of one call are distinct: two threads never write one entry)
hipError_t launch_gain_set(float* tgt, const int32_t* slots, const float* a, int32_t n_slots, hipStream_t s) {
    if (n_slots <= 0) return hipSuccess;
    if (!tgt || !slots || !a) return hipErrorInvalidValue;
    GainSetArgs g{};
    g.tgt = tgt;
    for (int32_t first = 0; first < n_slots; first += kSlotResetIds) {
        g.n = std::min<int32_t>(kSlotResetIds, n_slots - first);
        for (int32_t k = 0; k < g.n; ++k) { g.slot[k] = (unsigned short)slots[first + k]; g.a[k] = a[first + k]; }
        online_gain_set<<<noted(dim3(1)), kIoThreads, 0, s>>>(g);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_gain_commit(const float* tgt, const float* cur_old, float* cur_new, int32_t n_slots, int32_t slot, hipStream_t s) {
    if (n_slots <= 0) return hipSuccess;
    if (!tgt || !cur_old || !cur_new || cur_old == cur_new || slot >= n_slots) return hipErrorInvalidValue;
    online_gain_commit<<<noted(dim3(1)), kIoThreads, 0, s>>>(tgt, cur_old, cur_new, n_slots, slot);
    return hipGetLastError();
}

int64_t band_job_words(int32_t n, int32_t n_bands, int32_t rows) { return 2 * (int64_t)n + n_bands + 1 + (int64_t)rows * n_bands; }

hipError_t launch_band_expand(float* tab, int32_t FS, int32_t F, const int32_t* job, int32_t n, int32_t n_bands, int32_t rows, bool init,
                              hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!tab || !job || FS < F || F < 1 || n > 65535 || n_bands < 1 || n_bands > F || rows < 1) return hipErrorInvalidValue;
    const BandExpandArgs a{tab, job, FS, F, n, n_bands, rows, init ? 1 : 0};
    online_band_expand<<<noted(dim3((unsigned)ceil_div(FS, kIoThreads), (unsigned)n)), kIoThreads, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_band_commit(float* tab, int32_t FS, int32_t n_slots, int32_t slot, int mode, const int64_t* slot_start, hipStream_t s) {
    if (n_slots <= 0) return hipSuccess;
    if (!tab || FS < 1 || n_slots > 65535 || slot >= n_slots || mode < kBandCommit || mode > kBandCarry) return hipErrorInvalidValue;
    online_band_commit<<<noted(dim3((unsigned)ceil_div(FS, kIoThreads), (unsigned)(slot < 0 ? n_slots : 1))), kIoThreads, 0, s>>>(
        tab, FS, slot, mode, slot_start);
    return hipGetLastError();
}

// the gain fields of EmitArgs / LevelArgs from a caller's EmitGain (null: no gain, the fields stay zero)
template <typename Args> static hipError_t set_gain(Args& a, const EmitGain* gain) {
    if (!gain) return hipSuccess;
    if (gain->scalar) { a.gain = kGainScalar; a.a = gain->a; return hipSuccess; }
    if (!gain->a_tgt || gain->ramp < 0 || (gain->ramp > 0 && !gain->a_cur)) return hipErrorInvalidValue;
    a.gain = kGainTables; a.a_cur = gain->a_cur; a.a_tgt = gain->a_tgt; a.ramp = gain->ramp;
    return hipSuccess;
}

hipError_t launch_stream_emit(const float* bg, const float* hi, const float* lo, int64_t in_stream, const int64_t* slot_start,
                              int64_t pos0, int64_t hop, int32_t n_streams, int64_t n, int32_t ch, int dtype, const EmitDst* dsts,
                              int n_dsts, hipStream_t s, const EmitGain* gain, const float* bg_fg, const int64_t* live_len) {
    const int64_t count = (int64_t)n_streams * n * ch;
    if (count <= 0 || n_dsts <= 0) return hipSuccess;
    if (n_dsts > 2 || !bg || !hi) return hipErrorInvalidValue;
    EmitArgs a{};
    if (set_gain(a, gain) != hipSuccess) return hipErrorInvalidValue;
    a.bg = bg; a.bg_fg = bg_fg; a.hi = hi; a.lo = lo; a.in_stream = in_stream; a.count = count; a.per = n * ch; a.n_samples = n;
    a.slot_start = slot_start; a.pos0 = pos0; a.hop = hop; a.n_channels = ch; a.n_out = n_dsts; a.live_len = live_len;
    a.bg_only = live_len ? 1 : 0;
    for (int k = 0; k < n_dsts; ++k) if (dsts[k].which != REPET_OUT_BACKGROUND) a.bg_only = 0;
    // (the vector store of a dense destination: 16 bytes for F64 / F32, kEpt16 elements for the 16-bit types)
    const int vec_bytes = dtype == REPET_F64 || dtype == REPET_F32 ? 16 : 2 * kEpt16;
    for (int k = 0; k < n_dsts; ++k) {
        const IoGeo g{count, n, ch, dsts[k].strides[0], dsts[k].strides[1], dsts[k].strides[2]};
        a.out[k] = EmitOut{dsts[k].p, g.s_clip, g.s_sample, g.s_channel, dsts[k].which, noted_dense(k, is_dense(dsts[k].p, g, n_streams, vec_bytes))};
    }
    const dim3 grid16((unsigned)ceil_div(ceil_div(count, kEpt16), kIoThreads));
    switch (dtype) {
        case REPET_F64: devio_emit_f64<<<noted(dim3((unsigned)ceil_div(ceil_div(count, 2), kIoThreads))), kIoThreads, 0, s>>>(a); break;
        case REPET_F32: devio_emit_f32<<<noted(dim3((unsigned)ceil_div(ceil_div(count, 4), kIoThreads))), kIoThreads, 0, s>>>(a); break;
        case REPET_I16: devio_emit_i16<<<noted(grid16), kIoThreads, 0, s>>>(a); break;
        case REPET_F16: devio_emit_f16<<<noted(grid16), kIoThreads, 0, s>>>(a); break;
        case REPET_BF16: devio_emit_bf16<<<noted(grid16), kIoThreads, 0, s>>>(a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// elements of a tile of the level reduction: a multiple of the channel count, and of 4 where that fits (0: too many channels)
static int32_t level_tile(int32_t ch) {
    const int64_t both = std::lcm<int64_t>(4, ch);
    if (both <= kLevelSlots) return (int32_t)(kLevelSlots / both * both);
    return ch <= kLevelSlots ? kLevelSlots / ch * ch : 0;
}

int64_t stream_levels_partials(int32_t n_streams, int64_t n, int32_t ch) {
    const int64_t chunks = ceil_div(n, kLevelChunk);
    return chunks > 1 ? (int64_t)n_streams * ch * chunks * REPET_LEVEL_FIELDS : 0;
}

hipError_t launch_stream_levels(const float* bg, const float* hi, const float* lo, int64_t in_stream, const int64_t* slot_start,
                                int64_t pos0, int64_t hop, int32_t n_streams, int64_t n, int32_t ch, double* dst, double* partials,
                                hipStream_t s, const EmitGain* gain, const float* bg_fg, const int64_t* live_len) {
    if (n_streams <= 0 || ch <= 0) return hipSuccess;
    if (!dst) return hipErrorInvalidValue;
    const int64_t count = (int64_t)n_streams * n * ch;
    if (count <= 0) return hipMemsetAsync(dst, 0, (size_t)n_streams * ch * REPET_LEVEL_FIELDS * sizeof(double), s);
    const int64_t chunks = ceil_div(n, kLevelChunk);
    if (!bg || !hi || (chunks > 1 && !partials) || chunks > 0x7fffffff || n_streams > 65535) return hipErrorInvalidValue;
    LevelArgs a{};
    a.tile = level_tile(ch);
    if (a.tile <= 0) return hipErrorNotSupported;
    if (set_gain(a, gain) != hipSuccess) return hipErrorInvalidValue;
    a.bg = bg; a.bg_fg = bg_fg; a.hi = hi; a.lo = lo; a.in_stream = in_stream; a.per = n * ch;
    a.slot_start = slot_start; a.pos0 = pos0; a.hop = hop; a.n_channels = ch; a.n_chunks = (int32_t)chunks;
    a.dst = dst; a.partial = partials; a.live_len = live_len;
    devio_levels<<<noted(dim3((unsigned)chunks, (unsigned)n_streams)), kIoThreads, 0, s>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || chunks == 1) return e;
    devio_levels_fold<<<noted(dim3((unsigned)(n_streams * ch))), 64, 0, s>>>(partials, (int32_t)chunks, dst, live_len, ch);
    return hipGetLastError();
}

// two destinations of one emission must not share memory: their address ranges (first to last element) must not intersect
int check_disjoint(const void* p0, const int64_t* st0, const void* p1, const int64_t* st1, int elem_bytes, int32_t n_clips, int64_t n,
                   int32_t ch) {
    if ((int64_t)n_clips * n * ch <= 0) return REPET_OK;
    auto last = [&](const int64_t* st) { return (st[0] * (n_clips - 1) + st[1] * (n - 1) + st[2] * (ch - 1) + 1) * elem_bytes; };
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(p0), b0 = reinterpret_cast<uintptr_t>(p1);
    if (a0 < b0 + (uintptr_t)last(st1) && b0 < a0 + (uintptr_t)last(st0))
        return fail(REPET_ERR_BAD_ARG, "the two destinations overlap (their address ranges must not intersect)");
    return REPET_OK;
}

int dtype_bytes(int dtype) { return element_size(dtype); }

int check_emit_dtype(int dtype) {
    if (!element_size(dtype)) return fail(REPET_ERR_BAD_ARG, "the result is float64, float32, int16, float16 or bfloat16");
    return REPET_OK;
}

int check_strides(const int64_t* strides) {
    if (!strides) return fail(REPET_ERR_BAD_ARG, "strides is null");
    for (int k = 0; k < 3; ++k)
        if (strides[k] < 0) return fail(REPET_ERR_BAD_ARG, "negative stride (make the tensor contiguous first)");
    return REPET_OK;
}

// a destination whose elements do not overlap: with its dimensions of more than one element ordered by stride, each stride
// must step past everything the smaller ones span (a stride-0 `expand` view, or any other aliasing, would have several egress
// threads write different values to one address)
int check_no_overlap(const int64_t* strides, int32_t n_clips, int64_t n, int32_t ch) {
    const int64_t size[3] = {n_clips, n, ch};
    int order[3] = {0, 1, 2};
    std::sort(order, order + 3, [&](int a, int b) { return strides[a] < strides[b]; });
    int64_t span = 0;                                 // largest offset reachable through the dimensions taken so far
    for (int k : order) {
        if (size[k] <= 1) continue;
        if (strides[k] <= span) return fail(REPET_ERR_BAD_ARG, "the destination's elements overlap (an expanded or aliasing view)");
        span += strides[k] * (size[k] - 1);
    }
    return REPET_OK;
}

int check_background_gain(float gain) {
    if (!(gain >= 0.f && gain <= 1.f)) return fail(REPET_ERR_BAD_ARG, "the background gain must lie in [0, 1] (NaN and infinities are refused)");
    return REPET_OK;
}

float background_gain_factor(float gain) { return (float)(1.0 - (double)gain); }

int ensure_io_events(repet_ctx* c) {
    if (!c->io_wait) HIP_TRY(hipEventCreateWithFlags(&c->io_wait, hipEventDisableTiming));
    if (!c->io_done) HIP_TRY(hipEventCreateWithFlags(&c->io_done, hipEventDisableTiming));
    return REPET_OK;
}

int wait_caller(repet_ctx* c, void* wait_stream, void* signal_stream) {
    const hipStream_t wait = static_cast<hipStream_t>(wait_stream), signal = static_cast<hipStream_t>(signal_stream);
    RP_TRY(ensure_io_events(c));
    HIP_TRY(hipEventRecord(c->io_wait, wait));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->io_wait, 0));
    if (signal != wait) {
        HIP_TRY(hipEventRecord(c->io_wait, signal));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->io_wait, 0));
    }
    return REPET_OK;
}

int signal_caller(repet_ctx* c, void* signal_stream) {
    HIP_TRY(hipEventRecord(c->io_done, c->stream));
    HIP_TRY(hipStreamWaitEvent(static_cast<hipStream_t>(signal_stream), c->io_done, 0));
    return REPET_OK;
}

hipError_t launch_tail_clear(float2* X, float* Mk, int64_t spec_stride, int64_t chan_stride, int32_t n_clips, int32_t ch, int64_t T,
                             int32_t FS, int32_t W, int32_t H, const int64_t* lengths_dev, int64_t longest_tail, hipStream_t s) {
    if (longest_tail <= 0 || n_clips <= 0) return hipSuccess;
    if (!X || !lengths_dev || n_clips > 65535 || ch < 1 || ch > 65535 || (FS & 3)) return hipErrorInvalidValue;
    const int64_t groups = ceil_div(longest_tail * FS, (int64_t)kIoThreads * 4);
    const int64_t x_cap = std::max<int64_t>(1, kMaxIoGroups / ((int64_t)n_clips * ch));
    devio_tail_clear<<<noted(dim3((unsigned)std::min(groups, x_cap), (unsigned)n_clips, (unsigned)ch)), kIoThreads, 0, s>>>(
        X, Mk, spec_stride, chan_stride, T, FS, W, H, lengths_dev);
    return hipGetLastError();
}

// the strided ingest, equal clips (len_dev null) or ragged ones
hipError_t launch_ingest(const void* src, int dtype, int32_t n_clips, int64_t n, int32_t ch, const int64_t strides[3], float* hi,
                         float* lo, unsigned int* flag, const int64_t* len_dev, hipStream_t s) {
    const int64_t count = n * ch * n_clips;
    if (count <= 0) return hipSuccess;
    if (!src || !hi || (dtype == REPET_F64 && !lo) || (reinterpret_cast<uintptr_t>(hi) & 15) ||
        (dtype == REPET_F64 && (reinterpret_cast<uintptr_t>(lo) & 15)) || dtype < REPET_F32 || dtype > REPET_BF16)
        return hipErrorInvalidValue;
    IoGeo g{count, n, ch, strides[0], strides[1], strides[2]};
    const int vec_bytes = dtype == REPET_F64 ? 16 : 4 * element_size(dtype);
    const int dense = noted_dense(0, is_dense(src, g, n_clips, vec_bytes));
    const dim3 grid((unsigned)ceil_div(ceil_div(count, 4), kIoThreads));
    if (len_dev) switch (dtype) {
        case REPET_F64: devio_ingest_ragged_f64<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const double*>(src), g, dense, hi, lo, flag, len_dev); break;
        case REPET_F32: devio_ingest_ragged_f32<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const float*>(src), g, dense, hi, nullptr, flag, len_dev); break;
        case REPET_I16: devio_ingest_ragged_i16<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const int16_t*>(src), g, dense, hi, nullptr, flag, len_dev); break;
        case REPET_F16: devio_ingest_ragged_f16<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const Half*>(src), g, dense, hi, nullptr, flag, len_dev); break;
        default: devio_ingest_ragged_bf16<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const BHalf*>(src), g, dense, hi, nullptr, flag, len_dev); break;
    }
    else switch (dtype) {
        case REPET_F64: devio_ingest_f64<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const double*>(src), g, dense, hi, lo, flag); break;
        case REPET_F32: devio_ingest_f32<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const float*>(src), g, dense, hi, nullptr, flag); break;
        case REPET_I16: devio_ingest_i16<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const int16_t*>(src), g, dense, hi, nullptr, flag); break;
        case REPET_F16: devio_ingest_f16<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const Half*>(src), g, dense, hi, nullptr, flag); break;
        default: devio_ingest_bf16<<<noted(grid), kIoThreads, 0, s>>>(static_cast<const BHalf*>(src), g, dense, hi, nullptr, flag); break;
    }
    return hipGetLastError();
}

// the upload through it: equal clips (lengths null) or ragged ones (lengths[b] in [0, n], checked by the caller, not all equal to n)
static int upload_strided(repet_ctx* c, const void* src, int dtype, int32_t n_clips, int64_t n, int32_t ch, const int64_t strides[3],
                          const int64_t* lengths, void* wait_stream) {
    if (!c) return fail(REPET_ERR_BAD_ARG, "ctx is null");
    if (n < 0 || ch < 1 || n_clips < 1) return fail(REPET_ERR_BAD_ARG, "audio_signal must be (number_samples, number_channels)");
    if (dtype < REPET_F32 || dtype > REPET_BF16) return fail(REPET_ERR_BAD_ARG, "unsupported dtype");
    RP_TRY(check_strides(strides));
    const int64_t count = n * ch * n_clips;
    if (count > 0 && !src) return fail(REPET_ERR_BAD_ARG, "null argument");
    DeviceGuard guard(c->device);
    HIP_TRY(c->audio.ensure(std::max<size_t>((size_t)count * sizeof(float), 256)));
    HIP_TRY(c->out.ensure(std::max<size_t>((size_t)count * sizeof(float), 256)));
    if (dtype == REPET_F64) HIP_TRY(c->audio_lo.ensure(std::max<size_t>((size_t)count * sizeof(float), 256)));
    // the producer of `src` is the caller's stream: the context's stream starts the ingest behind what it has enqueued so far
    RP_TRY(wait_caller(c, wait_stream, wait_stream));
    // a float64 host upload of this context may still have its remainder plane on the way into audio_lo (copy stream): the
    // ingest must land after it, not under it. (lo_in_flight stays set: the host has not seen the copy finish, and the ring's
    // remainder buffer must not be refilled before it has -- StagingRing waits for lo_done then.)
    if (c->ring.lo_in_flight) HIP_TRY(hipStreamWaitEvent(c->stream, c->ring.lo_done, 0));
    const int64_t* len_dev = nullptr;
    if (lengths) {
        // the table travels in the arguments of a small launch (the online_slot_set pattern: no copy the host would wait for)
        HIP_TRY(c->clip_len_dev.ensure((size_t)n_clips * sizeof(int64_t)));
        std::vector<int32_t> ids((size_t)n_clips);
        std::iota(ids.begin(), ids.end(), 0);
        HIP_TRY(launch_slot_set(c->clip_len_dev.as<int64_t>(), ids.data(), lengths, n_clips, c->stream));
        len_dev = c->clip_len_dev.as<int64_t>();
    }
    const bool refuse = !c->strict;
    unsigned int* flag = nullptr;
    if (refuse) {
        HIP_TRY(c->nonfinite_word.ensure(sizeof(unsigned int)));
        flag = c->nonfinite_word.as<unsigned int>();
        HIP_TRY(hipMemsetAsync(flag, 0, sizeof(unsigned int), c->stream));
    }
    if (count > 0)
        HIP_TRY(launch_ingest(src, dtype, n_clips, n, ch, strides, c->audio.as<float>(), c->audio_lo.as<float>(), flag, len_dev, c->stream));
    if (refuse) {
        // the refusal mode's one host wait: the flag word decides whether the clip is accepted
        unsigned int seen = 0;
        HIP_TRY(hipMemcpyAsync(&seen, flag, sizeof(seen), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (seen) {
            c->n_channels = 0;
            return fail(REPET_ERR_BAD_ARG, "audio_signal contains NaN or infinite samples");
        }
    }
    // as repet_ctx_upload_device_split leaves it: device planes are not scanned (strict mode never reads the flag word),
    // what they hold is computed on; a float64 source always brings its remainder plane
    c->has_lo = dtype == REPET_F64 && count > 0;
    c->input_not_finite = false;
    c->input_unscanned = true;
    c->n_samples = n; c->n_channels = ch; c->n_clips = n_clips; c->clip_base = 0;
    c->win_total = 0; c->win_offset = 0; c->clip_len.clear();
    if (lengths) c->clip_len.assign(lengths, lengths + n_clips);
    c->result_shaped = false;
    return REPET_OK;
}

}  // namespace repet_eng

extern "C" {

int repet_ctx_upload_device_strided(repet_ctx* c, const void* src, int dtype, int32_t n_clips, int64_t n, int32_t ch,
                                    const int64_t strides[3], void* wait_stream) {
    return upload_strided(c, src, dtype, n_clips, n, ch, strides, nullptr, wait_stream);
}

int repet_ctx_upload_device_ragged(repet_ctx* c, const void* src, int dtype, int32_t n_clips, int64_t n, int32_t ch,
                                   const int64_t strides[3], const int64_t* lengths, void* wait_stream) {
    if (!c) return fail(REPET_ERR_BAD_ARG, "ctx is null");
    if (!lengths) return fail(REPET_ERR_BAD_ARG, "lengths is null");
    if (n < 0 || ch < 1 || n_clips < 1) return fail(REPET_ERR_BAD_ARG, "audio_signal must be (number_samples, number_channels)");
    if (n_clips > 65535) return fail(REPET_ERR_LIMIT, "a ragged batch holds at most 65535 clips");
    bool equal = true;
    for (int32_t b = 0; b < n_clips; ++b) {
        if (lengths[b] < 0 || lengths[b] > n)
            return fail(REPET_ERR_BAD_ARG, "lengths[" + std::to_string(b) + "] = " + std::to_string(lengths[b]) + " lies outside [0, n_samples]");
        equal = equal && lengths[b] == n;
    }
    // (every clip as long as the pitch: the equal-length path, its kernels and its bits)
    return upload_strided(c, src, dtype, n_clips, n, ch, strides, equal ? nullptr : lengths, wait_stream);
}

int repet_ctx_clip_lengths(repet_ctx* c, int64_t* out, int32_t capacity, int32_t* n_written) {
    if (!c || !n_written || capacity < 0 || (capacity > 0 && !out)) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (c->n_channels < 1) return fail(REPET_ERR_BAD_ARG, "no clip uploaded");
    *n_written = c->n_clips;
    for (int32_t b = 0; b < c->n_clips && b < capacity; ++b) out[b] = c->ragged() ? c->clip_len[(size_t)b] : c->n_samples;
    return REPET_OK;
}

int repet_emit_dtype_supported(int dtype) { return element_size(dtype) ? 1 : 0; }

int repet_ctx_set_online_start(repet_ctx* c, int32_t start_frames) {
    if (!c) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (start_frames < 0) return fail(REPET_ERR_BAD_ARG, "start_frames must be >= 0 (0: buffer_frames, the reference)");
    c->online_start = start_frames;
    return REPET_OK;
}

int repet_ctx_select_result(repet_ctx* c, int which) {
    if (!c) return fail(REPET_ERR_BAD_ARG, "ctx is null");
    if (which < REPET_OUT_BACKGROUND || which > REPET_OUT_MIXTURE)
        return fail(REPET_ERR_BAD_ARG, "which must be REPET_OUT_BACKGROUND, REPET_OUT_FOREGROUND or REPET_OUT_MIXTURE");
    c->result_which = which;
    return REPET_OK;
}

int repet_ctx_set_background_gain(repet_ctx* c, float gain) {
    if (!c) return fail(REPET_ERR_BAD_ARG, "ctx is null");
    RP_TRY(check_background_gain(gain));
    c->result_gain = gain != 0.f;                       // (0, the default: the foreground as it always was, by the path it always took)
    c->result_a = background_gain_factor(gain);
    return REPET_OK;
}

int repet_ctx_download_device_strided(repet_ctx* c, void* dst, int dtype, const int64_t strides[3], void* signal_stream) {
    if (!c) return fail(REPET_ERR_BAD_ARG, "ctx is null");
    if (c->n_channels < 1) return fail(REPET_ERR_BAD_ARG, "no clip uploaded");
    RP_TRY(check_emit_dtype(dtype));
    RP_TRY(check_strides(strides));
    RP_TRY(check_no_overlap(strides, c->n_clips, c->n_samples, c->n_channels));
    const int64_t count = c->n_samples * c->n_channels * c->n_clips;
    if (count > 0 && !dst) return fail(REPET_ERR_BAD_ARG, "null argument");
    DeviceGuard guard(c->device);
    // the destination belongs to the caller's stream: what that stream has enqueued up to now (a pending reader of a block the
    // caching allocator has just handed out again, the caller's own writes to `dst`) comes before the egress writes it
    RP_TRY(wait_caller(c, signal_stream, signal_stream));
    if (count > 0 && (c->result_which != REPET_OUT_BACKGROUND || c->ragged())) {      // (a ragged background: the emission's select)
        // foreground / mixture: the resident samples and, where a float64 upload left them, their remainders beside the result
        if (c->has_lo && c->ring.lo_in_flight) HIP_TRY(hipStreamWaitEvent(c->stream, c->ring.lo_done, 0));
        EmitDst d{dst, c->result_which, {strides[0], strides[1], strides[2]}};
        EmitGain gain;
        gain.scalar = true; gain.a = c->result_a;
        HIP_TRY(launch_stream_emit(c->out.as<float>(), c->audio.as<float>(), c->has_lo ? c->audio_lo.as<float>() : nullptr,
                                   c->n_samples * c->n_channels, nullptr, 0, 1, c->n_clips, c->n_samples, c->n_channels, dtype, &d, 1,
                                   c->stream, c->result_gain ? &gain : nullptr, c->shaped_bg(), c->live_len()));
    } else if (count > 0) {
        HIP_TRY(launch_stream_egress(c->out.as<float>(), c->n_clips, c->n_samples, c->n_channels, dst, dtype, strides, c->stream));
    }
    // the caller's stream continues behind the egress
    return signal_caller(c, signal_stream);
}

int repet_ctx_result_levels_device(repet_ctx* c, void* dst, void* signal_stream) {
    if (!c) return fail(REPET_ERR_BAD_ARG, "ctx is null");
    if (c->n_channels < 1) return fail(REPET_ERR_BAD_ARG, "no clip uploaded");
    if (!dst) return fail(REPET_ERR_BAD_ARG, "null destination");
    DeviceGuard guard(c->device);
    // the destination belongs to the caller's stream, as in repet_ctx_download_device_strided
    RP_TRY(wait_caller(c, signal_stream, signal_stream));
    const int64_t count = c->n_samples * c->n_channels * c->n_clips;
    if (count > 0 && c->has_lo && c->ring.lo_in_flight) HIP_TRY(hipStreamWaitEvent(c->stream, c->ring.lo_done, 0));
    const int64_t partials = stream_levels_partials(c->n_clips, c->n_samples, c->n_channels);
    if (partials > 0) HIP_TRY(c->levels_ws.ensure((size_t)partials * sizeof(double)));
    EmitGain gain;
    gain.scalar = true; gain.a = c->result_a;
    // every sample of a resident clip is live: no table, one hop
    const hipError_t e = launch_stream_levels(c->out.as<float>(), c->audio.as<float>(), c->has_lo ? c->audio_lo.as<float>() : nullptr,
                                              c->n_samples * c->n_channels, nullptr, 0, 1, c->n_clips, c->n_samples, c->n_channels,
                                              static_cast<double*>(dst), partials > 0 ? c->levels_ws.as<double>() : nullptr, c->stream,
                                              c->result_gain ? &gain : nullptr, c->shaped_bg(), c->live_len());
    if (e == hipErrorNotSupported) return fail(REPET_ERR_LIMIT, "too many channels for the level reduction");
    HIP_TRY(e);
    return signal_caller(c, signal_stream);
}

}  // extern "C"
