// stage-level exports and the accessors of the last run's integer intermediates (see engine.h for the map of the engine's files)
#include "engine.h"
#include "fft_path.h"

using namespace repet;
using namespace repet_eng;

extern "C" {

// ---- stage-level exports ---------------------------------------------------------------------------

int repet_stft(repet_ctx* c, const float* x, int64_t n, const float* window, int32_t W, int32_t H, int32_t centred,
               float* spec_out, int64_t n_frames) {
    if (!c || !x || !window || !spec_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (H < 1) return fail(REPET_ERR_BAD_ARG, "step length must be >= 1");
    DeviceGuard guard(c->device);
    const float2* tw = nullptr;
    RP_TRY(upload_twiddle_only(c, W, &tw));
    const int64_t T = repet_frame_count(n, W, H, centred);
    if (T != n_frames) return fail(REPET_ERR_BAD_ARG, "n_frames does not match repet_frame_count");
    const Geo g = make_geo(W, H, T, 1);
    HIP_TRY(c->tmp_a.ensure(std::max<size_t>((size_t)n * sizeof(float), 256)));
    HIP_TRY(c->tmp_b.ensure((size_t)W * sizeof(float)));
    HIP_TRY(c->X.ensure((size_t)g.chan_stride * sizeof(float2)));
    HIP_TRY(c->V.ensure((size_t)g.chan_stride * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(c->tmp_a.p, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->tmp_b.p, window, (size_t)W * sizeof(float), hipMemcpyHostToDevice, c->stream));
    StftArgs a{};
    a.audio = c->tmp_a.as<float>(); a.n_samples = n; a.n_channels = 1; a.sample_offset = 0;
    a.window = c->tmp_b.as<float>(); a.twiddle = tw; a.W = W; a.H = H; a.T = T; a.FS = g.FS; a.centred = centred;
    a.X = c->X.as<float2>(); a.V = c->V.as<float>(); a.chan_stride = g.chan_stride;
    HIP_TRY(launch_stft(a, c->stream));
    if (T > 0)
        HIP_TRY(hipMemcpy2DAsync(spec_out, (size_t)g.F * sizeof(float2), c->X.p, (size_t)g.FS * sizeof(float2),
                                 (size_t)g.F * sizeof(float2), T, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return REPET_OK;
}

int repet_istft(repet_ctx* c, const float* spec, int64_t T, const float* window, int32_t W, int32_t H, float* y_out,
                int64_t n_out) {
    if (!c || !spec || !window || !y_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (H < 1 || H > W) return fail(REPET_ERR_BAD_ARG, "bad step length");
    DeviceGuard guard(c->device);
    const float2* tw = nullptr;
    RP_TRY(upload_twiddle_only(c, W, &tw));
    const int64_t want = T * H - (W - H);                           // repet.py:1079,1098
    if (n_out != want) return fail(REPET_ERR_BAD_ARG, "n_out must be T*H - (W-H)");
    const Geo g = make_geo(W, H, T, 1);
    HIP_TRY(c->X.ensure((size_t)g.chan_stride * sizeof(float2)));
    HIP_TRY(hipMemsetAsync(c->X.p, 0, (size_t)g.chan_stride * sizeof(float2), c->stream));
    HIP_TRY(hipMemcpy2DAsync(c->X.p, (size_t)g.FS * sizeof(float2), spec, (size_t)g.F * sizeof(float2),
                             (size_t)g.F * sizeof(float2), T, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c->frames.ensure((size_t)T * W * sizeof(float)));
    HIP_TRY(c->tmp_a.ensure(std::max<size_t>((size_t)n_out * sizeof(float), 256)));
    IstftArgs ia{};
    ia.Y = c->X.as<float2>(); ia.chan_stride = g.chan_stride; ia.n_channels = 1; ia.T = T; ia.FS = g.FS; ia.W = W;
    ia.twiddle = tw; ia.frames = c->frames.as<float>();
    HIP_TRY(launch_istft_frames(ia, c->stream));
    double cola = 0;
    for (int i = 0; i < W; i += H) cola += window[i];
    OlaArgs oa{};
    oa.frames = c->frames.as<float>(); oa.n_channels = 1; oa.T = T; oa.W = W; oa.H = H; oa.trim = W - H;
    oa.out = c->tmp_a.as<float>(); oa.n_out = n_out; oa.out_offset = 0; oa.scale = (float)(1.0 / cola);
    HIP_TRY(launch_overlap_add(oa, c->stream));
    HIP_TRY(hipMemcpyAsync(y_out, c->tmp_a.p, (size_t)n_out * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return REPET_OK;
}

// ---- stage entries of the PRODUCTION launchers (tests/test_gpu_stft_stages.py) -----------------------------------------
// repet_stft above is launch_stft for one mono clip and repet_istft runs two kernels nothing else launches. These two run
// launch_stft / launch_istft_ola with everything the pipelines pass them -- channels, batches, offsets, the side products,
// mask plane or model, the cross-fade of `extended` -- on buffers laid out by make_geo, with the kernel family as an
// argument (fft_path.h), and say which kernel ran. Diagnostic exports like the ones below: not part of repet_hip.h.
namespace {
struct Scratch { DevBuf b; ~Scratch() { b.release(); } };

int report_launch(const FftLaunch& info, char* kernel_out, int32_t kernel_cap, int64_t* launch_out) {
    if (kernel_out && kernel_cap > 0) { std::strncpy(kernel_out, info.kernel, (size_t)kernel_cap - 1); kernel_out[kernel_cap - 1] = 0; }
    if (launch_out) {
        const int64_t v[8] = {info.family, info.run, info.rounds, info.slots, info.workgroups, info.units, info.launches, 0};
        std::memcpy(launch_out, v, sizeof(v));
    }
    return REPET_OK;
}
bool window_length_ok(int W) { return W >= 64 && W <= 8192 && !(W & (W - 1)); }
}  // namespace

// audio (n_total, C) fp32 interleaved; n_batch clips of n_samples samples, the first at sample_offset, batch_sample_stride
// apart. want: 1 Vm, 2 Vn, 4 P, 8 Vh (with Vn), 16 Ph + Ph_inv (register kernel only). Every device buffer is filled with
// the byte `prefill` first. geo_out[6] = T, Tpad, rows = Tpad + pad rows, F, FS, chan_stride; with X_out null only geo_out
// is filled (the caller sizes its arrays from it): X (B, C, rows, FS, 2), V (B, C, rows, FS), Vm / Vn / P (B, Tpad, FS),
// Vh / Ph (B, Tpad, 2 FS) halves, Ph_inv (B, Tpad). launch_out[8] = family, run, rounds, slots, workgroups, units, launches, 0.
int repet_debug_stft_stage(repet_ctx* c, const float* audio, int64_t n_total, int32_t C, const float* window, int32_t W, int32_t H,
                           int32_t centred, int64_t sample_offset, int64_t n_samples, int32_t n_batch, int64_t batch_sample_stride,
                           int32_t path, int32_t want, int32_t fix_infinite, int32_t prefill, int64_t* geo_out,
                           float* X_out, float* V_out, float* Vm_out, float* Vn_out, float* P_out, uint16_t* Vh_out, uint16_t* Ph_out,
                           float* Ph_inv_out, char* kernel_out, int32_t kernel_cap, int64_t* launch_out) {
    if (!c || !audio || !window || !geo_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (!window_length_ok(W)) return fail(REPET_ERR_LIMIT, "window length must be a power of two in [64, 8192]");
    if (H < 1 || H > W || C < 1 || C > 64 || n_batch < 1 || n_samples < 1 || sample_offset < 0 || batch_sample_stride < 0)
        return fail(REPET_ERR_BAD_ARG, "bad size");
    if (path < kFftPathAuto || path > kFftPathReg) return fail(REPET_ERR_BAD_ARG, "path: 0 as production picks, 1 block, 2 wave, 3 reg");
    if (sample_offset + (int64_t)(n_batch - 1) * batch_sample_stride + n_samples > n_total)
        return fail(REPET_ERR_BAD_ARG, "the clips do not fit into the audio buffer");
    if ((want & 8) && !(want & 2)) return fail(REPET_ERR_BAD_ARG, "the f16 planes of the unit rows come with the unit rows");
    if ((want & 16) && !reg_fft_supported(W, C, false, path)) return fail(REPET_ERR_BAD_ARG, "only the register kernel writes the row-scaled planes");
    const int64_t T = repet_frame_count(n_samples, W, H, centred);
    const Geo g = make_geo(W, H, T, C);
    const int64_t rows = g.chan_stride / g.FS, geo[6] = {T, g.Tpad, rows, g.F, g.FS, g.chan_stride};
    std::memcpy(geo_out, geo, sizeof(geo));
    if (!X_out) return REPET_OK;
    if (!V_out || ((want & 1) && !Vm_out) || ((want & 2) && !Vn_out) || ((want & 4) && !P_out) || ((want & 8) && !Vh_out) ||
        ((want & 16) && (!Ph_out || !Ph_inv_out)))
        return fail(REPET_ERR_BAD_ARG, "null output");
    DeviceGuard guard(c->device);
    const float2* tw = nullptr;
    RP_TRY(upload_twiddle_only(c, W, &tw));
    const size_t spec = (size_t)n_batch * C * g.chan_stride, mean = (size_t)n_batch * g.Tpad * g.FS;
    Scratch in, win, X, V, Vm, Vn, P, Vh, Ph, Pi;
    HIP_TRY(in.b.ensure((size_t)n_total * C * sizeof(float)));
    HIP_TRY(win.b.ensure((size_t)W * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(in.b.p, audio, (size_t)n_total * C * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(win.b.p, window, (size_t)W * sizeof(float), hipMemcpyHostToDevice, c->stream));
    auto filled = [&](Scratch& s, bool on, size_t bytes) -> int {
        if (!on) return REPET_OK;
        HIP_TRY(s.b.ensure(bytes));
        HIP_TRY(hipMemsetAsync(s.b.p, prefill & 255, bytes, c->stream));
        return REPET_OK;
    };
    RP_TRY(filled(X, true, spec * sizeof(float2)));
    RP_TRY(filled(V, true, spec * sizeof(float)));
    RP_TRY(filled(Vm, want & 1, mean * sizeof(float)));
    RP_TRY(filled(Vn, want & 2, mean * sizeof(float)));
    RP_TRY(filled(P, want & 4, mean * sizeof(float)));
    RP_TRY(filled(Vh, want & 8, mean * 2 * sizeof(uint16_t)));
    RP_TRY(filled(Ph, want & 16, mean * 2 * sizeof(uint16_t)));
    RP_TRY(filled(Pi, want & 16, (size_t)n_batch * g.Tpad * sizeof(float)));
    StftArgs a{};
    a.audio = in.b.as<float>(); a.n_samples = n_samples; a.n_channels = C; a.sample_offset = sample_offset;
    a.window = win.b.as<float>(); a.twiddle = tw; a.W = W; a.H = H; a.T = T; a.FS = g.FS; a.centred = centred;
    a.X = X.b.as<float2>(); a.V = V.b.as<float>(); a.chan_stride = g.chan_stride;
    a.Vm = Vm.b.as<float>(); a.Vn = Vn.b.as<float>(); a.P = P.b.as<float>(); a.Vh = Vh.b.p;
    a.Ph = Ph.b.p; a.Ph_inv = Pi.b.as<float>(); a.batch_inv_stride = g.Tpad;
    a.n_batch = n_batch; a.batch_sample_stride = batch_sample_stride; a.batch_spec_stride = (int64_t)C * g.chan_stride;
    a.batch_mean_stride = g.Tpad * g.FS;
    FftLaunch info;
    hipError_t e = launch_stft(a, c->stream, path, &info);
    if (e == hipErrorInvalidValue) return fail(REPET_ERR_LIMIT, "the kernel family asked for does not take this shape");
    HIP_TRY(e);
    if (fix_infinite) HIP_TRY(launch_infinite_frames_fix(a, c->stream));
    auto back = [&](void* dst, const Scratch& s, bool on, size_t bytes) -> int {
        if (on) HIP_TRY(hipMemcpyAsync(dst, s.b.p, bytes, hipMemcpyDeviceToHost, c->stream));
        return REPET_OK;
    };
    RP_TRY(back(X_out, X, true, spec * sizeof(float2)));
    RP_TRY(back(V_out, V, true, spec * sizeof(float)));
    RP_TRY(back(Vm_out, Vm, want & 1, mean * sizeof(float)));
    RP_TRY(back(Vn_out, Vn, want & 2, mean * sizeof(float)));
    RP_TRY(back(P_out, P, want & 4, mean * sizeof(float)));
    RP_TRY(back(Vh_out, Vh, want & 8, mean * 2 * sizeof(uint16_t)));
    RP_TRY(back(Ph_out, Ph, want & 16, mean * 2 * sizeof(uint16_t)));
    RP_TRY(back(Ph_inv_out, Pi, want & 16, (size_t)n_batch * g.Tpad * sizeof(float)));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return report_launch(info, kernel_out, kernel_cap, launch_out);
}

// Y (n_spec, C, T, F, 2) half spectra, hop W / 2. One of: nothing; M (n_spec, C, T, F), a mask plane; model (n_spec, C,
// model_rows, F) with periods[n_spec] and cutoff (register kernel only). n_batch = 0: one clip at out_offset; n_batch > 0:
// the segment-batch fields as run_original fills them (slot s: spectra batch_local0 + s batch_step, segment j = batch_first
// + s batch_step written at out_offset + j batch_out_stride). `out` (out_len, C) is the caller's pre-filled buffer: it goes
// to the device as it is and comes back whole.
int repet_debug_istft_stage(repet_ctx* c, const float* Y, int32_t n_spec, int32_t C, int64_t T, int32_t W, int64_t trim, int64_t n_out,
                            int64_t out_offset, float scale, const float* M, const float* model, const int32_t* periods,
                            int32_t model_rows, int32_t cutoff, int32_t accumulate_weighted, int64_t fade_in, int64_t fade_out,
                            int32_t n_batch, int32_t batch_first, int32_t batch_step, int32_t batch_total, int32_t batch_local0,
                            int64_t batch_out_stride, int64_t overlap, int32_t path, float* out, int64_t out_len,
                            char* kernel_out, int32_t kernel_cap, int64_t* launch_out) {
    if (!c || !Y || !out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (!window_length_ok(W)) return fail(REPET_ERR_LIMIT, "window length must be a power of two in [64, 8192]");
    if (n_spec < 1 || C < 1 || C > 64 || T < 1 || trim < 0 || n_out < 0 || out_offset < 0 || out_len < 1 || fade_in < 0 || fade_out < 0 ||
        overlap < 0 || batch_out_stride < 0 || accumulate_weighted < 0 || accumulate_weighted > 2 || cutoff < 0)
        return fail(REPET_ERR_BAD_ARG, "bad size");
    if (path < kFftPathAuto || path > kFftPathReg) return fail(REPET_ERR_BAD_ARG, "path: 0 as production picks, 1 block, 2 wave, 3 reg");
    if (M && model) return fail(REPET_ERR_BAD_ARG, "a mask plane or a model, not both");
    if (model) {
        if (!periods || model_rows < 1) return fail(REPET_ERR_BAD_ARG, "a model needs its periods");
        for (int i = 0; i < n_spec; ++i)
            if (periods[i] < 1 || periods[i] > model_rows) return fail(REPET_ERR_BAD_ARG, "a period outside the model's rows");
    }
    // every sample the launch may touch lies inside `out`, every spectrum it may read inside Y
    if (n_batch < 0) return fail(REPET_ERR_BAD_ARG, "bad batch");
    if (n_batch == 0) {
        if (out_offset + n_out > out_len) return fail(REPET_ERR_BAD_ARG, "the span does not fit into the output buffer");
    } else {
        if (batch_step < 1 || batch_first < 0 || batch_local0 < 0) return fail(REPET_ERR_BAD_ARG, "bad batch");
        const int64_t last_local = batch_local0 + (int64_t)(n_batch - 1) * batch_step, last_j = batch_first + (int64_t)(n_batch - 1) * batch_step;
        if (last_local >= n_spec || last_j >= batch_total) return fail(REPET_ERR_BAD_ARG, "the batch reaches past its spectra or its segment count");
        if (out_offset + last_j * batch_out_stride + n_out > out_len) return fail(REPET_ERR_BAD_ARG, "the span does not fit into the output buffer");
    }
    DeviceGuard guard(c->device);
    const float2* tw = nullptr;
    RP_TRY(upload_twiddle_only(c, W, &tw));
    const Geo g = make_geo(W, W / 2, T, C);
    const size_t planes = (size_t)n_spec * C, spec = planes * g.chan_stride;
    Scratch Yd, Md, Wd, Pd, Od;
    HIP_TRY(Yd.b.ensure(spec * sizeof(float2)));
    HIP_TRY(hipMemsetAsync(Yd.b.p, 0, spec * sizeof(float2), c->stream));
    for (size_t p = 0; p < planes; ++p)
        HIP_TRY(hipMemcpy2DAsync(Yd.b.as<float2>() + p * g.chan_stride, (size_t)g.FS * sizeof(float2), Y + p * (size_t)T * g.F * 2,
                                 (size_t)g.F * sizeof(float2), (size_t)g.F * sizeof(float2), T, hipMemcpyHostToDevice, c->stream));
    if (M) {
        HIP_TRY(Md.b.ensure(spec * sizeof(float)));
        HIP_TRY(hipMemsetAsync(Md.b.p, 0, spec * sizeof(float), c->stream));
        for (size_t p = 0; p < planes; ++p)
            HIP_TRY(hipMemcpy2DAsync(Md.b.as<float>() + p * g.chan_stride, (size_t)g.FS * sizeof(float), M + p * (size_t)T * g.F,
                                     (size_t)g.F * sizeof(float), (size_t)g.F * sizeof(float), T, hipMemcpyHostToDevice, c->stream));
    }
    if (model) {
        const size_t cells = planes * model_rows * g.FS;
        HIP_TRY(Wd.b.ensure(cells * sizeof(float)));
        HIP_TRY(hipMemsetAsync(Wd.b.p, 0, cells * sizeof(float), c->stream));
        HIP_TRY(hipMemcpy2DAsync(Wd.b.p, (size_t)g.FS * sizeof(float), model, (size_t)g.F * sizeof(float), (size_t)g.F * sizeof(float),
                                 planes * model_rows, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(Pd.b.ensure((size_t)n_spec * sizeof(int32_t)));
        HIP_TRY(hipMemcpyAsync(Pd.b.p, periods, (size_t)n_spec * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    const size_t out_bytes = (size_t)out_len * C * sizeof(float);
    HIP_TRY(Od.b.ensure(out_bytes));
    HIP_TRY(hipMemcpyAsync(Od.b.p, out, out_bytes, hipMemcpyHostToDevice, c->stream));
    IstftOlaArgs a{};
    a.Y = Yd.b.as<float2>(); a.M = M ? Md.b.as<float>() : nullptr; a.chan_stride = g.chan_stride; a.n_channels = C; a.T = T; a.FS = g.FS; a.W = W;
    a.twiddle = tw; a.trim = trim; a.out = Od.b.as<float>(); a.n_out = n_out; a.out_offset = out_offset; a.scale = scale;
    a.accumulate_weighted = accumulate_weighted; a.fade_in = fade_in; a.fade_out = fade_out;
    a.n_batch = n_batch; a.batch_first = batch_first; a.batch_step = batch_step; a.batch_total = batch_total; a.batch_local0 = batch_local0;
    a.batch_spec_stride = (int64_t)C * g.chan_stride; a.batch_out_stride = batch_out_stride; a.overlap = overlap;
    if (model) {
        const ModelRef mr{Wd.b.as<float>(), Pd.b.as<int32_t>(), (int64_t)C * model_rows * g.FS, (int64_t)model_rows * g.FS, cutoff};
        apply_model(a, c, &mr);
    }
    FftLaunch info;
    hipError_t e = launch_istft_ola(a, c->stream, path, &info);
    if (e == hipErrorInvalidValue) return fail(REPET_ERR_LIMIT, "the kernel family asked for does not take this shape or mask form");
    HIP_TRY(e);
    HIP_TRY(hipMemcpyAsync(out, Od.b.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return report_launch(info, kernel_out, kernel_cap, launch_out);
}

// ---- stage entries of the banded Gram and of the period chain (tests/test_gpu_gram_band_stages.py) ----------------------
// exec_gram_band -- the second half of run_gram_band -- on rows laid out as the pipelines lay them out: B clips of T rows,
// clip_stride_rows apart (at least Tpad = round_up(T, 128); more is the online handle's case), pitch FS, pad rows and pad
// bins zero. form: 0 as gram_band_form picks from (unit_rows, lookback, planes_ready), 1 fp32, 2 f16 row-scaled planes, 3
// f16 unit rows, 4 the same in the look-back layout. Every device buffer -- the rows' gaps, the band, the context's planes
// and row inverses -- is filled with the byte `prefill` first. geo_out[8] = Tpad, FS, LP, the form that ran, band_on_f16,
// band_lookback, the tile list's length, 0; with band_out null nothing runs and geo_out holds the form that WOULD run (the
// only use of planes_ready: there are no planes to hand over). band_out (B, clip_stride_rows, LP); forms 2 - 4: planes_out
// (B, Tpad, 2 FS) halves; form 2: inv_out (B, Tpad).
int repet_debug_gram_band_stage(repet_ctx* c, const float* rows, int32_t B, int64_t T, int32_t F, int32_t n_lags, int64_t clip_stride_rows,
                                int32_t form, int32_t unit_rows, int32_t lookback, int32_t planes_ready, int32_t prefill, int64_t* geo_out,
                                float* band_out, uint16_t* planes_out, float* inv_out, char* kernel_out, int32_t kernel_cap) {
    if (!c || !geo_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (B < 1 || T < 1 || F < 1 || n_lags < 1 || n_lags > T) return fail(REPET_ERR_BAD_ARG, "bad size");
    if (form < kBandAuto || form > kBandF16UnitLookback)
        return fail(REPET_ERR_BAD_ARG, "form: 0 as production picks, 1 fp32, 2 f16 row-scaled, 3 f16 unit rows, 4 f16 unit rows look-back");
    const int FS = (int)round_up(F, kFreqAlign), LP = (int)round_up(n_lags, 64);
    const int64_t Tpad = round_up(T, kTile);
    if (clip_stride_rows < Tpad) return fail(REPET_ERR_BAD_ARG, "the clip stride is at least round_up(T, 128) rows");
    DeviceGuard guard(c->device);
    const int64_t a_stride = clip_stride_rows * FS, band_stride = clip_stride_rows * LP;
    const int ran = form != kBandAuto ? form
                                      : gram_band_form(c, T, FS, n_lags, unit_rows != 0, B, a_stride, planes_ready != 0, lookback != 0);
    const int2* tiles; int n_tiles;
    RP_TRY(get_tiles(c, T, gram_band_diagonals(n_lags), &tiles, &n_tiles));
    int64_t geo[8] = {Tpad, FS, LP, ran, ran != kBandF32, ran == kBandF16UnitLookback, n_tiles, 0};
    if (!band_out) { std::memcpy(geo_out, geo, sizeof(geo)); return REPET_OK; }
    if (!rows || (ran != kBandF32 && !planes_out) || (ran == kBandF16Rows && !inv_out)) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (planes_ready) return fail(REPET_ERR_BAD_ARG, "planes_ready only asks for the choice: this entry has no planes to hand over");
    if (ran == kBandF16Rows && B > 1 && clip_stride_rows != Tpad)
        return fail(REPET_ERR_BAD_ARG, "the row-scaled planes of a batch are packed clip by clip: the stride is round_up(T, 128)");
    const size_t a_count = (size_t)a_stride * (B - 1) + (size_t)Tpad * FS, band_count = (size_t)band_stride * B;
    Scratch Ad, Bd;
    HIP_TRY(Ad.b.ensure(a_count * sizeof(float)));
    HIP_TRY(Bd.b.ensure(band_count * sizeof(float)));
    HIP_TRY(hipMemsetAsync(Ad.b.p, prefill & 255, a_count * sizeof(float), c->stream));
    HIP_TRY(hipMemsetAsync(Bd.b.p, prefill & 255, band_count * sizeof(float), c->stream));
    for (int b = 0; b < B; ++b)
        RP_TRY(h2d_pitched(c, Ad.b.as<float>() + (size_t)b * a_stride, FS, rows + (size_t)b * T * F, T, F, Tpad));
    if (ran != kBandF32) {                            // what exec_gram_band will ask for: it then finds the buffers large enough
        HIP_TRY(c->Vh.ensure(a_count * 4));
        HIP_TRY(hipMemsetAsync(c->Vh.p, prefill & 255, a_count * 4, c->stream));
        if (ran == kBandF16Rows) {
            HIP_TRY(c->amax.ensure((size_t)Tpad * B * sizeof(float)));
            HIP_TRY(hipMemsetAsync(c->amax.p, prefill & 255, (size_t)Tpad * B * sizeof(float), c->stream));
        }
    }
    RP_TRY(exec_gram_band(c, ran, Ad.b.as<float>(), T, FS, Bd.b.as<float>(), n_lags, LP, B, a_stride, band_stride, false));
    geo[4] = c->band_on_f16; geo[5] = c->band_lookback;
    std::memcpy(geo_out, geo, sizeof(geo));
    HIP_TRY(hipMemcpyAsync(band_out, Bd.b.p, band_count * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (ran != kBandF32) {
        const size_t clip_halves = (size_t)Tpad * FS * 2;
        for (int b = 0; b < B; ++b)
            HIP_TRY(hipMemcpyAsync(planes_out + (size_t)b * clip_halves, c->Vh.as<uint16_t>() + (size_t)b * a_stride * 2, clip_halves * sizeof(uint16_t),
                                   hipMemcpyDeviceToHost, c->stream));
        if (ran == kBandF16Rows)
            HIP_TRY(hipMemcpyAsync(inv_out, c->amax.p, (size_t)Tpad * B * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (kernel_out && kernel_cap > 0) {
        std::strncpy(kernel_out, ran == kBandF32 ? "gram_kernel<GRAM_BAND>" : "gram_f16_kernel<true>", (size_t)kernel_cap - 1);
        kernel_out[kernel_cap - 1] = 0;
    }
    return REPET_OK;
}

// ---- stage entry of the full similarity matrix (tests/test_gpu_gram_full_stages.py) --------------------------------------
// exec_gram_full -- the second half of run_gram_full -- on rows (T, F) laid out as `sim` lays out its unit rows: Tpad =
// round_up(T, 128) rows of pitch FS, pad rows and pad bins zero; S (T, TS = round_up(T, 64)); the records (T, 3, seg_pitch).
// The rows are taken as given (the caller passes unit rows); normalise: launch_unit_rows runs on them first and vn_out
// (Tpad, FS) brings back what it wrote. form: 0 as gram_full_form picks for unit rows, 1 fp32, 2 f16-split 128 x 128, 3
// f16-split 256 x 256 -- 2 and 3 at any T (the 2 048-frame threshold belongs to the choice). records: 0 none, 1 as `sim`
// gets them (the epilogue of form 3, a pass over S otherwise), 2 always by launch_segment_maxima. Every device buffer -- the
// rows, S, the records, the context's planes out to round_up(T, 256) rows -- is filled with the byte `prefill` first, so with
// form 3 the plane rows [Tpad, round_up(T, 256)) still hold it when the kernel reads them. geo_out[8] = Tpad, FS, TS,
// seg_pitch, the form that ran, the records' source (0 none, 1 epilogue, 2 pass over S), the tile list's padded length, the
// tile edge; with s_out null nothing runs and geo_out holds what WOULD run. s_out (T, TS) whole, guard columns included;
// top_out / second_out / at_out (T, seg_pitch); planes_out (round_up(T, tile edge), 2 FS) halves for forms 2 and 3.
// REPET_ERR_BAD_ARG: a null argument, T < 1, F < 1, form or records out of range; REPET_ERR_LIMIT: T > 4096 or F > 8192 (the
// entry's own caps: S is T x TS floats).
int repet_debug_gram_full_stage(repet_ctx* c, const float* rows, int64_t T, int32_t F, int32_t form, int32_t records, int32_t normalise,
                                int32_t prefill, int64_t* geo_out, float* s_out, float* top_out, float* second_out, int32_t* at_out,
                                uint16_t* planes_out, float* vn_out, char* kernel_out, int32_t kernel_cap) {
    if (!c || !geo_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (T < 1 || F < 1) return fail(REPET_ERR_BAD_ARG, "bad size");
    if (T > 4096 || F > 8192) return fail(REPET_ERR_LIMIT, "this entry takes at most 4096 rows of at most 8192 bins");
    if (form < kFullAuto || form > kFullF16Big)
        return fail(REPET_ERR_BAD_ARG, "form: 0 as production picks, 1 fp32, 2 f16 128 x 128 tiles, 3 f16 256 x 256 tiles");
    if (records < 0 || records > 2) return fail(REPET_ERR_BAD_ARG, "records: 0 none, 1 as production gets them, 2 by the pass over S");
    const int FS = (int)round_up(F, kFreqAlign);
    const int64_t Tpad = round_up(T, kTile), TS = round_up(T, 64);
    const int seg_pitch = segment_pitch((int)TS);
    const int ran = form != kFullAuto ? form : gram_full_form(T, true);
    const int edge = ran == kFullF16Big ? gram_big_tile() : kTile;
    const int64_t plane_rows = round_up(T, edge);
    const int source = records == 0 ? 0 : (records == 1 && ran == kFullF16Big && gram_segments_in_epilogue()) ? 1 : 2;
    std::vector<int2> list;
    const int64_t geo[8] = {Tpad, FS, TS, seg_pitch, ran, source, gram_tile_list((int)ceil_div(T, edge), 1 << 30, &list), edge};
    std::memcpy(geo_out, geo, sizeof(geo));
    if (!s_out) return REPET_OK;
    if (!rows || (records && (!top_out || !second_out || !at_out)) || (ran != kFullF32 && !planes_out) || (normalise && !vn_out))
        return fail(REPET_ERR_BAD_ARG, "null argument");
    DeviceGuard guard(c->device);
    const size_t a_bytes = (size_t)Tpad * FS * sizeof(float), s_bytes = (size_t)T * TS * sizeof(float);
    const size_t seg_bytes = (size_t)T * 3 * seg_pitch * sizeof(float), plane_bytes = (size_t)round_up(T, gram_big_tile()) * FS * 4;
    Scratch Ad, Sd, Gd, Raw;
    HIP_TRY(Ad.b.ensure(a_bytes));
    HIP_TRY(Sd.b.ensure(s_bytes));
    HIP_TRY(Gd.b.ensure(seg_bytes));
    HIP_TRY(hipMemsetAsync(Ad.b.p, prefill & 255, a_bytes, c->stream));
    HIP_TRY(hipMemsetAsync(Sd.b.p, prefill & 255, s_bytes, c->stream));
    HIP_TRY(hipMemsetAsync(Gd.b.p, prefill & 255, seg_bytes, c->stream));
    if (ran != kFullF32) {                            // more than exec_gram_full will ask for: it then finds the buffer large enough
        HIP_TRY(c->Vh.ensure(plane_bytes));
        HIP_TRY(hipMemsetAsync(c->Vh.p, prefill & 255, plane_bytes, c->stream));
    }
    if (normalise) {
        HIP_TRY(Raw.b.ensure((size_t)T * F * sizeof(float)));
        HIP_TRY(hipMemcpyAsync(Raw.b.p, rows, (size_t)T * F * sizeof(float), hipMemcpyHostToDevice, c->stream));
        if (Tpad > T) HIP_TRY(hipMemsetAsync(Ad.b.as<float>() + (size_t)T * FS, 0, (size_t)(Tpad - T) * FS * sizeof(float), c->stream));
        HIP_TRY(launch_unit_rows(Raw.b.as<float>(), Ad.b.as<float>(), T, F, FS, c->stream));
    } else {
        RP_TRY(h2d_pitched(c, Ad.b.as<float>(), FS, rows, T, F, Tpad));
    }
    RP_TRY(exec_gram_full(c, ran, Ad.b.as<float>(), T, FS, Sd.b.as<float>(), TS, false, records ? Gd.b.as<float>() : nullptr, seg_pitch,
                          nullptr, source == 1));
    HIP_TRY(hipMemcpyAsync(s_out, Sd.b.p, s_bytes, hipMemcpyDeviceToHost, c->stream));
    if (records)
        for (int plane = 0; plane < 3; ++plane) {
            void* dst = plane == 0 ? (void*)top_out : plane == 1 ? (void*)second_out : (void*)at_out;
            HIP_TRY(hipMemcpy2DAsync(dst, (size_t)seg_pitch * 4, Gd.b.as<float>() + (size_t)plane * seg_pitch, (size_t)3 * seg_pitch * 4,
                                     (size_t)seg_pitch * 4, (size_t)T, hipMemcpyDeviceToHost, c->stream));
        }
    if (ran != kFullF32)
        HIP_TRY(hipMemcpyAsync(planes_out, c->Vh.p, (size_t)plane_rows * FS * 4, hipMemcpyDeviceToHost, c->stream));
    if (normalise) HIP_TRY(hipMemcpyAsync(vn_out, Ad.b.p, a_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (kernel_out && kernel_cap > 0) {
        std::strncpy(kernel_out, ran == kFullF32 ? "gram_kernel<GRAM_FULL>" : ran == kFullF16 ? "gram_f16_kernel<false>" : "gram_f16_big_pipe_kernel",
                     (size_t)kernel_cap - 1);
        kernel_out[kernel_cap - 1] = 0;
    }
    return REPET_OK;
}

// run_band_window_sum -> launch_periods -> (T_expand > 0) launch_expand_periods on a band (B, T, LP) given as it is, LP a
// multiple of 64: window w covers frames [start0 + w step, + len). beat_out (B, n_windows, LP), win_periods_out (B,
// n_windows), frame_periods_out (T_expand) from the first clip's window periods (null with T_expand = 0). The beat rows
// are filled with `prefill` first: a lag from n_lags on keeps it.
int repet_debug_band_periods_stage(repet_ctx* c, const float* band, int32_t B, int64_t T, int32_t LP, int32_t n_lags, int32_t n_freq,
                                   int64_t start0, int64_t step, int64_t len, int32_t n_windows, int32_t lo, int32_t hi,
                                   int32_t n_lags_for_clamp, int64_t T_expand, int32_t prefill, float* beat_out,
                                   int32_t* win_periods_out, int32_t* frame_periods_out) {
    if (!c || !band || !beat_out || !win_periods_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (B < 1 || T < 1 || LP < 64 || (LP & 63) || n_lags < 1 || n_lags > LP || n_freq < 1 || step < 0 || len < 1 || n_windows < 1 ||
        lo < 0 || T_expand < 0 || (T_expand > 0 && (!frame_periods_out || step < 1)))
        return fail(REPET_ERR_BAD_ARG, "bad size");
    const int h = std::min(hi, n_lags_for_clamp / 3);
    if (h <= lo) return fail(REPET_ERR_TOO_SHORT, "attempt to get argmax of an empty sequence");
    if (h > LP) return fail(REPET_ERR_BAD_ARG, "the searched lags end past the beat rows");
    if (T_expand > 0 && ceil_div(T_expand, step) > n_windows) return fail(REPET_ERR_BAD_ARG, "T_expand needs more windows");
    DeviceGuard guard(c->device);
    const size_t band_count = (size_t)B * T * LP, beat_count = (size_t)B * n_windows * LP;
    Scratch Bd, Be, Wp, Fp;
    HIP_TRY(Bd.b.ensure(band_count * sizeof(float)));
    HIP_TRY(Be.b.ensure(beat_count * sizeof(float)));
    HIP_TRY(Wp.b.ensure((size_t)B * n_windows * sizeof(int32_t)));
    HIP_TRY(Fp.b.ensure(std::max<size_t>((size_t)T_expand * sizeof(int32_t), 256)));
    HIP_TRY(hipMemcpyAsync(Bd.b.p, band, band_count * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(Be.b.p, prefill & 255, beat_count * sizeof(float), c->stream));
    HIP_TRY(hipMemsetAsync(Wp.b.p, prefill & 255, (size_t)B * n_windows * sizeof(int32_t), c->stream));
    HIP_TRY(hipMemsetAsync(Fp.b.p, prefill & 255, std::max<size_t>((size_t)T_expand * sizeof(int32_t), 256), c->stream));
    RP_TRY(run_band_window_sum(c, Bd.b.as<float>(), T, LP, n_lags, n_freq, start0, step, len, n_windows, Be.b.as<float>(), LP, B,
                               (int64_t)T * LP, (int64_t)n_windows * LP));
    HIP_TRY(launch_periods(Be.b.as<float>(), B * n_windows, LP, n_lags_for_clamp, lo, hi, Wp.b.as<int32_t>(), c->stream));
    if (T_expand > 0) {
        HIP_TRY(launch_expand_periods(Wp.b.as<int32_t>(), n_windows, (int32_t)step, T_expand, lo, Fp.b.as<int32_t>(), c->stream));
        HIP_TRY(hipMemcpyAsync(frame_periods_out, Fp.b.p, (size_t)T_expand * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(beat_out, Be.b.p, beat_count * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(win_periods_out, Wp.b.p, (size_t)B * n_windows * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return REPET_OK;
}

static int stage_matrix_in(repet_ctx* c, DevBuf& buf, const float* host, int64_t T, int F, int FS, int64_t Tpad) {
    HIP_TRY(buf.ensure((size_t)Tpad * FS * sizeof(float)));
    return h2d_pitched(c, buf.as<float>(), FS, host, T, F, Tpad);
}

int repet_selfsim(repet_ctx* c, const float* v, int64_t T, int32_t F, float* s_out) {
    if (!c || !v || !s_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    DeviceGuard guard(c->device);
    const int FS = (int)round_up(F, kFreqAlign);
    const int64_t Tpad = round_up(T, kTile), TS = round_up(T, 64);
    HIP_TRY(c->tmp_a.ensure((size_t)T * F * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(c->tmp_a.p, v, (size_t)T * F * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c->Vn.ensure((size_t)Tpad * FS * sizeof(float)));
    HIP_TRY(hipMemsetAsync(c->Vn.p, 0, (size_t)Tpad * FS * sizeof(float), c->stream));
    HIP_TRY(launch_unit_rows(c->tmp_a.as<float>(), c->Vn.as<float>(), T, F, FS, c->stream));
    HIP_TRY(c->S.ensure((size_t)T * TS * sizeof(float)));
    RP_TRY(run_gram_full(c, c->Vn.as<float>(), T, FS, c->S.as<float>(), TS, true));   // unit rows: same kernel as `sim`
    return d2h_pitched(c, s_out, c->S.as<float>(), TS, T, T);
}

int repet_selfsim_records(repet_ctx* c, const float* v, int64_t T, int32_t F, float* s_out, float* max_out, float* second_out,
                          int32_t* at_out) {
    if (!c || !v || !s_out || !max_out || !second_out || !at_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    DeviceGuard guard(c->device);
    const int FS = (int)round_up(F, kFreqAlign);
    const int64_t Tpad = round_up(T, kTile), TS = round_up(T, 64);
    const int seg_pitch = segment_pitch((int)TS), n_seg = (int)ceil_div(T, kSegWidth);
    HIP_TRY(c->tmp_a.ensure((size_t)T * F * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(c->tmp_a.p, v, (size_t)T * F * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c->Vn.ensure((size_t)Tpad * FS * sizeof(float)));
    HIP_TRY(hipMemsetAsync(c->Vn.p, 0, (size_t)Tpad * FS * sizeof(float), c->stream));
    HIP_TRY(launch_unit_rows(c->tmp_a.as<float>(), c->Vn.as<float>(), T, F, FS, c->stream));
    HIP_TRY(c->S.ensure((size_t)T * TS * sizeof(float)));
    HIP_TRY(c->seg.ensure((size_t)T * 3 * seg_pitch * sizeof(float)));
    // the records as `sim` gets them: from the 256 x 256 kernel's epilogue for clips of 2 048 frames and more, else by a pass over S
    RP_TRY(run_gram_full(c, c->Vn.as<float>(), T, FS, c->S.as<float>(), TS, true, false, c->seg.as<float>(), seg_pitch));
    RP_TRY(d2h_pitched(c, s_out, c->S.as<float>(), TS, T, T));
    for (int plane = 0; plane < 3; ++plane) {
        void* dst = plane == 0 ? (void*)max_out : plane == 1 ? (void*)second_out : (void*)at_out;
        HIP_TRY(hipMemcpy2DAsync(dst, (size_t)n_seg * 4, c->seg.as<float>() + (size_t)plane * seg_pitch, (size_t)3 * seg_pitch * 4,
                                 (size_t)n_seg * 4, (size_t)T, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return REPET_OK;
}

int repet_similarity(repet_ctx* c, const float* a, int64_t TA, const float* b, int64_t TB, int32_t F, float* s_out) {
    if (!c || !a || !b || !s_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (TA < 1 || TB < 1 || F < 1) return fail(REPET_ERR_BAD_ARG, "bad size");
    DeviceGuard guard(c->device);
    const int FS = (int)round_up(F, kFreqAlign);
    const int64_t TApad = round_up(TA, kTile), TBpad = round_up(TB, kTile), pitch = round_up(TB, 4);
    HIP_TRY(c->tmp_a.ensure((size_t)std::max(TA, TB) * F * sizeof(float)));
    HIP_TRY(c->Vn.ensure((size_t)TApad * FS * sizeof(float)));
    HIP_TRY(c->P.ensure((size_t)TBpad * FS * sizeof(float)));
    HIP_TRY(hipMemsetAsync(c->Vn.p, 0, (size_t)TApad * FS * sizeof(float), c->stream));
    HIP_TRY(hipMemsetAsync(c->P.p, 0, (size_t)TBpad * FS * sizeof(float), c->stream));
    HIP_TRY(hipMemcpyAsync(c->tmp_a.p, a, (size_t)TA * F * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_unit_rows(c->tmp_a.as<float>(), c->Vn.as<float>(), TA, F, FS, c->stream));
    HIP_TRY(hipMemcpyAsync(c->tmp_a.p, b, (size_t)TB * F * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_unit_rows(c->tmp_a.as<float>(), c->P.as<float>(), TB, F, FS, c->stream));
    HIP_TRY(c->S.ensure((size_t)TA * pitch * sizeof(float)));
    HIP_TRY(launch_matmul_nt(c->Vn.as<float>(), TA, c->P.as<float>(), TB, FS, c->S.as<float>(), pitch, c->stream));
    return d2h_pitched(c, s_out, c->S.as<float>(), pitch, TA, TB);
}

int repet_acorr(repet_ctx* c, const float* x, int32_t n_rows, int32_t n_cols, float* ac_out) {
    if (!c || !x || !ac_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (n_rows < 1 || n_cols < 1) return fail(REPET_ERR_BAD_ARG, "bad size");
    DeviceGuard guard(c->device);
    const size_t bytes = (size_t)n_rows * n_cols * sizeof(float);
    HIP_TRY(c->tmp_a.ensure(bytes));
    HIP_TRY(c->tmp_c.ensure(bytes));
    HIP_TRY(hipMemcpyAsync(c->tmp_a.p, x, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_acorr(c->tmp_a.as<float>(), n_rows, n_cols, n_cols, c->tmp_c.as<float>(), c->stream));
    HIP_TRY(hipMemcpyAsync(ac_out, c->tmp_c.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return REPET_OK;
}

int repet_beat_spectrum(repet_ctx* c, const float* p, int64_t T, int32_t F, float* beat_out, int32_t n_lags) {
    if (!c || !p || !beat_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (n_lags < 1 || n_lags > T) return fail(REPET_ERR_BAD_ARG, "n_lags must be in [1, T]");
    DeviceGuard guard(c->device);
    const int FS = (int)round_up(F, kFreqAlign);
    const int64_t Tpad = round_up(T, kTile);
    const int LP = (int)round_up(n_lags, 64);
    RP_TRY(stage_matrix_in(c, c->P, p, T, F, FS, Tpad));
    HIP_TRY(c->band.ensure((size_t)Tpad * LP * sizeof(float)));
    HIP_TRY(c->beat.ensure((size_t)LP * sizeof(float)));
    RP_TRY(run_gram_band(c, c->P.as<float>(), T, FS, c->band.as<float>(), n_lags, LP));
    RP_TRY(run_band_window_sum(c, c->band.as<float>(), T, LP, n_lags, F, 0, 0, T, 1, c->beat.as<float>(), LP, 1, 0, 0));
    return d2h_pitched(c, beat_out, c->beat.as<float>(), LP, 1, n_lags);
}

int repet_beat_spectrogram(repet_ctx* c, const float* p, int64_t T, int32_t F, int32_t Ls, int32_t Hs, float* beat_out) {
    if (!c || !p || !beat_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (Ls < 1 || Hs < 1) return fail(REPET_ERR_BAD_ARG, "bad segment length/step");
    DeviceGuard guard(c->device);
    const int FS = (int)round_up(F, kFreqAlign);
    const int64_t Tpad = round_up(T, kTile);
    const int LP = (int)round_up(Ls, 64);
    const int n_win = (int)ceil_div(T, Hs);
    RP_TRY(stage_matrix_in(c, c->P, p, T, F, FS, Tpad));
    HIP_TRY(c->band.ensure((size_t)Tpad * LP * sizeof(float)));
    HIP_TRY(hipMemsetAsync(c->band.p, 0, (size_t)Tpad * LP * sizeof(float), c->stream));
    HIP_TRY(c->beat.ensure((size_t)n_win * LP * sizeof(float)));
    RP_TRY(run_gram_band(c, c->P.as<float>(), T, FS, c->band.as<float>(), Ls, LP));
    const int64_t left = Ls / 2;                                     // ceil((Ls-1)/2)
    RP_TRY(run_band_window_sum(c, c->band.as<float>(), T, LP, Ls, F, -left, Hs, Ls, n_win, c->beat.as<float>(), LP, 1, 0, 0));
    std::vector<float> win((size_t)n_win * Ls);
    RP_TRY(d2h_pitched(c, win.data(), c->beat.as<float>(), LP, n_win, Ls));
    // replicate with the reference's hole (repet.py:1194-1204): frame i+Hs-1 of each step stays zero
    std::memset(beat_out, 0, (size_t)T * Ls * sizeof(float));
    for (int w = 0; w < n_win; ++w) {
        const int64_t i = (int64_t)w * Hs;
        const int64_t end = std::min<int64_t>(i + Hs - 1, T);
        std::memcpy(beat_out + i * Ls, win.data() + (size_t)w * Ls, (size_t)Ls * sizeof(float));
        for (int64_t t = i; t < end; ++t) std::memcpy(beat_out + t * Ls, win.data() + (size_t)w * Ls, (size_t)Ls * sizeof(float));
    }
    return REPET_OK;
}

int repet_periods(repet_ctx* c, const float* beat, int32_t n_cols, int32_t n_lags, int32_t lo, int32_t hi, int32_t* out) {
    if (!c || !beat || !out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (std::min(hi, n_lags / 3) <= lo) return fail(REPET_ERR_TOO_SHORT, "attempt to get argmax of an empty sequence");
    DeviceGuard guard(c->device);
    HIP_TRY(c->beat.ensure((size_t)n_cols * n_lags * sizeof(float)));
    HIP_TRY(c->periods.ensure((size_t)n_cols * sizeof(int32_t)));
    HIP_TRY(hipMemcpyAsync(c->beat.p, beat, (size_t)n_cols * n_lags * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_periods(c->beat.as<float>(), n_cols, n_lags, n_lags, lo, hi, c->periods.as<int32_t>(), c->stream));
    HIP_TRY(hipMemcpyAsync(out, c->periods.p, (size_t)n_cols * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return REPET_OK;
}

int repet_local_maxima(repet_ctx* c, const float* m, int32_t n_rows, int32_t n_cols, float min_value, int32_t d,
                       int32_t number, int32_t* idx_out, int32_t* count_out) {
    if (!c || !m || !idx_out || !count_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (n_rows < 1 || n_cols < 1 || number < 1 || d < 0) return fail(REPET_ERR_BAD_ARG, "bad size");
    DeviceGuard guard(c->device);
    const int64_t pitch = round_up(n_cols, 4);
    HIP_TRY(c->S.ensure((size_t)n_rows * pitch * sizeof(float)));
    RP_TRY(h2d_pitched(c, c->S.as<float>(), pitch, m, n_rows, n_cols, n_rows));
    HIP_TRY(c->idx.ensure((size_t)n_rows * number * sizeof(int32_t)));
    HIP_TRY(c->cnt.ensure((size_t)n_rows * sizeof(int32_t)));
    float* seg = nullptr;
    const int seg_pitch = segment_pitch((int)pitch);
    if (local_maxima_segments_apply(n_cols, d, pitch, 0, 1)) {
        HIP_TRY(c->seg.ensure((size_t)n_rows * 3 * seg_pitch * sizeof(float)));
        seg = c->seg.as<float>();
        HIP_TRY(launch_segment_maxima(c->S.as<float>(), n_rows, n_cols, pitch, seg, seg_pitch, c->stream));
    }
    hipError_t e = launch_local_maxima(c->S.as<float>(), n_rows, 0, n_cols, pitch, 0, min_value, d, number,
                                       c->idx.as<int32_t>(), number, c->cnt.as<int32_t>(), c->stream, 0, nullptr, nullptr, nullptr,
                                       nullptr, seg, seg_pitch);
    if (e == hipErrorInvalidValue) return fail(REPET_ERR_LIMIT, "row too long for the peak-picking kernel");
    HIP_TRY(e);
    HIP_TRY(hipMemcpyAsync(idx_out, c->idx.p, (size_t)n_rows * number * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(count_out, c->cnt.p, (size_t)n_rows * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return REPET_OK;
}

static int stage_mask_common(repet_ctx* c, const float* v, int64_t T, int F, MaskArgs* m, int* FS_out) {
    const int FS = (int)round_up(F, kFreqAlign);
    RP_TRY(stage_matrix_in(c, c->V, v, T, F, FS, T + kPadRows));
    HIP_TRY(launch_fill_pad_rows(c->V.as<float>(), (T + kPadRows) * FS, 1, T, FS, c->stream));
    HIP_TRY(c->tmp_c.ensure((size_t)T * FS * sizeof(float)));
    HIP_TRY(hipMemsetAsync(c->tmp_c.p, 0, (size_t)T * FS * sizeof(float), c->stream));
    *m = MaskArgs{};
    m->V = c->V.as<float>(); m->chan_stride = (T + kPadRows) * FS; m->n_channels = 1; m->T = T; m->F = F; m->FS = FS;
    m->X = nullptr; m->mask = c->tmp_c.as<float>(); m->cutoff = 0; m->pad_row = T;
    *FS_out = FS;
    return REPET_OK;
}

int repet_mask_period(repet_ctx* c, const float* v, int64_t T, int32_t F, int32_t period, float* mask_out) {
    if (!c || !v || !mask_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (period < 1) return fail(REPET_ERR_BAD_ARG, "period must be >= 1");
    DeviceGuard guard(c->device);
    MaskArgs m; int FS;
    RP_TRY(stage_mask_common(c, v, T, F, &m, &FS));
    HIP_TRY(launch_mask_period(m, nullptr, period, period, c->stream));
    return d2h_pitched(c, mask_out, c->tmp_c.as<float>(), FS, T, F);
}

int repet_mask_adaptive(repet_ctx* c, const float* v, int64_t T, int32_t F, const int32_t* periods, int32_t order,
                        float* mask_out) {
    if (!c || !v || !periods || !mask_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (order < 1) return fail(REPET_ERR_BAD_ARG, "filter_order must be >= 1");
    DeviceGuard guard(c->device);
    MaskArgs m; int FS;
    RP_TRY(stage_mask_common(c, v, T, F, &m, &FS));
    HIP_TRY(c->periods.ensure((size_t)T * sizeof(int32_t)));
    HIP_TRY(hipMemcpyAsync(c->periods.p, periods, (size_t)T * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_mask_adaptive(m, c->periods.as<int32_t>(), order, c->stream));
    return d2h_pitched(c, mask_out, c->tmp_c.as<float>(), FS, T, F);
}

int repet_mask_sim(repet_ctx* c, const float* v, int64_t T, int32_t F, const int32_t* idx, const int32_t* count,
                   int32_t number, float* mask_out) {
    if (!c || !v || !idx || !count || !mask_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    DeviceGuard guard(c->device);
    MaskArgs m; int FS;
    RP_TRY(stage_mask_common(c, v, T, F, &m, &FS));
    const int KP = std::max(number, kMinIdxPitch);
    HIP_TRY(c->idx.ensure((size_t)T * KP * sizeof(int32_t)));
    HIP_TRY(c->cnt.ensure((size_t)T * sizeof(int32_t)));
    HIP_TRY(hipMemsetAsync(c->idx.p, 0, (size_t)T * KP * sizeof(int32_t), c->stream));
    HIP_TRY(hipMemcpy2DAsync(c->idx.p, (size_t)KP * sizeof(int32_t), idx, (size_t)number * sizeof(int32_t),
                             (size_t)number * sizeof(int32_t), T, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->cnt.p, count, (size_t)T * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_mask_sim(m, c->idx.as<int32_t>(), KP, c->cnt.as<int32_t>(), 0, number, c->stream));
    return d2h_pitched(c, mask_out, c->tmp_c.as<float>(), FS, T, F);
}

int repet_mask_sim_ranked(repet_ctx* c, const float* v, int64_t T, int32_t F, const int32_t* idx, const int32_t* count,
                          int32_t number, int32_t path, float* mask_out, uint32_t* median_codes_out) {
    if (!c || !v || !idx || !count || !mask_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (path != 1 && path != 2) return fail(REPET_ERR_BAD_ARG, "path: 1 packed network on rank codes, 2 bit-sliced selection");
    const int n_cols = F - 1;
    if (F <= 128 || (n_cols & 127) || !rank_columns_supported(T) || number < 2 || number > 128)
        return fail(REPET_ERR_LIMIT, "rank-domain median: 1024 < n_frames <= 30720, n_freq - 1 a multiple of 128, lists of 2..128 entries");
    if (path == 2 && !mask_sim_bits_supported(T, 1, n_cols, number)) return fail(REPET_ERR_LIMIT, "bit-sliced selection: n_freq - 1 a power of two, at most 2048");
    DeviceGuard guard(c->device);
    MaskArgs m; int FS;
    RP_TRY(stage_mask_common(c, v, T, F, &m, &FS));
    const int64_t rows = T + kPadRows, vs_pitch = round_up(T, 32);
    HIP_TRY(c->R.ensure((size_t)rows * FS * sizeof(unsigned short)));
    c->r_pads_ptr = nullptr;                              // this export lays R out differently
    HIP_TRY(launch_fill_rank_pad_rows(c->R.as<unsigned short>(), rows * FS, 1, T, FS, c->stream));
    HIP_TRY(c->Vs.ensure((size_t)n_cols * vs_pitch * sizeof(float)));
    HIP_TRY(c->rank_codes.ensure((size_t)n_cols * vs_pitch * sizeof(unsigned short)));
    RankArgs a{};
    a.V = c->V.as<float>(); a.chan_stride = rows * FS; a.n_channels = 1; a.T = T; a.FS = FS; a.n_cols = n_cols;
    a.R = path == 2 ? nullptr : c->R.as<unsigned short>(); a.r_chan_stride = rows * FS; a.Vs = c->Vs.as<float>(); a.vs_pitch = vs_pitch;
    a.codes = c->rank_codes.as<unsigned short>();
    if (path == 2) {
        a.n_planes = code_planes_for(T);
        HIP_TRY(c->code_planes.ensure((size_t)T * a.n_planes * 64 * sizeof(unsigned)));
        a.P = c->code_planes.as<unsigned>();
        HIP_TRY(c->median_codes.ensure((size_t)rows * FS * sizeof(unsigned)));
        HIP_TRY(hipMemsetAsync(c->median_codes.p, 0, (size_t)rows * FS * sizeof(unsigned), c->stream));
        m.median_codes = c->median_codes.as<unsigned>();
    }
    HIP_TRY(launch_rank_columns(a, c->stream));
    m.R = a.R; m.r_chan_stride = a.r_chan_stride; m.Vs = a.Vs; m.vs_pitch = vs_pitch; m.n_rank_cols = n_cols;
    m.P = a.P; m.n_planes = a.n_planes;
    const int KP = std::max(number, kMinIdxPitch);
    HIP_TRY(c->idx.ensure((size_t)T * KP * sizeof(int32_t)));
    HIP_TRY(c->cnt.ensure((size_t)T * sizeof(int32_t)));
    HIP_TRY(hipMemsetAsync(c->idx.p, 0, (size_t)T * KP * sizeof(int32_t), c->stream));
    HIP_TRY(hipMemcpy2DAsync(c->idx.p, (size_t)KP * sizeof(int32_t), idx, (size_t)number * sizeof(int32_t),
                             (size_t)number * sizeof(int32_t), T, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->cnt.p, count, (size_t)T * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_mask_sim(m, c->idx.as<int32_t>(), KP, c->cnt.as<int32_t>(), 0, number, c->stream));
    if (median_codes_out) {
        if (path != 2) return fail(REPET_ERR_BAD_ARG, "median codes exist on path 2 only");
        HIP_TRY(hipMemcpy2DAsync(median_codes_out, (size_t)n_cols * 4, c->median_codes.p, (size_t)FS * 4, (size_t)n_cols * 4, T,
                                 hipMemcpyDeviceToHost, c->stream));
    }
    return d2h_pitched(c, mask_out, c->tmp_c.as<float>(), FS, T, F);
}

// ---- stage entry of the production mask launchers (tests/test_gpu_mask_stages.py) --------------------------------------
// The four exports above fix one channel, one clip, no cutoff, no X, a host period, first_frame = frame0 = 0 and pad_row = T:
// no pipeline launches the kernels that way. This one lays V (and X) out as make_geo does -- FS = round_up(F, 32), Tpad =
// round_up(T, 128), Tpad + kPadRows rows per channel, pad_row = Tpad, clips C * chan_stride apart --, runs launch_fill_pad_rows
// over all B * C planes as ensure_spectra does and then exactly ONE of launch_mask_period (kind 0), launch_mask_adaptive (1)
// and launch_mask_sim (2) with a MaskArgs the caller controls. V (B, C, T, F), X (nullable; B, C, T, F, 2). want: 1 the mask
// plane, 2 X in place, 4 the model (period only, and then nothing else: the kernel writes nothing else). Every device buffer
// -- V and X outside the caller's cells, the mask plane, the model, the median codes -- holds the byte `prefill` before the
// launch, and every output comes back whole: mask / X (B, C, Tpad + kPadRows, FS), model (B, C, T / 3 + 2, FS), codes (C, Tpad +
// kPadRows, FS). Everything a kernel indexes with is checked on the host first: bad input is REPET_ERR_BAD_ARG, a shape the
// median path asked for does not take REPET_ERR_LIMIT, never an out-of-range gather.
//   period    periods null: the host period `period_host`; else B device periods, min_period <= periods[b] <= T / 3 + 2
//   adaptive  periods (T), order
//   sim       idx (B, rows, width), cnt (B, rows), rows >= T - first_frame list rows numbered from first_frame; idx_pitch >= max(128,
//             width), any alignment; slot_start (nullable, B) + slot_bias; median_path 0 floats, 1 packed network on rank
//             codes, 2 bit-sliced selection, 3 the bit-sliced selection with the Nyquist bin in the ranked column of bin 1, as
//             exec_sim runs it (RankArgs / MaskArgs::swap_col = 1, swap_bin = F - 1; cutoff >= 1 and parts = 1, else
//             REPET_ERR_BAD_ARG: the lookups write that bin) (1 .. 3: B = 1, first_frame = 0; the column sort runs on all C
//             channels, with the calls of run_rank_columns)
// geo_out[8] = Tpad, rows per channel, FS, chan_stride, model rows, 0, 0, 0. launch_out[16] = net, flag, parts, grid x y z,
// Nyquist net, preload, grid x y z, 1 if mask_from_codes_kernel ran behind the selection, 0...; kernel_out / nyquist_out: the
// template names (MaskLaunch, common.h).
int repet_debug_mask_stage(repet_ctx* c, int32_t kind, const float* V, const float* X, int32_t B, int32_t C, int64_t T, int32_t F,
                           int32_t cutoff, int32_t prefill, int32_t want, int32_t period_host, const int32_t* periods,
                           int32_t min_period, int32_t order, const int32_t* idx, const int32_t* cnt, int64_t rows, int32_t width,
                           int64_t first_frame, int32_t max_count, int64_t frame0, int64_t frame_end, int32_t parts,
                           const int64_t* slot_start, int64_t slot_bias, int32_t idx_pitch, int32_t median_path, int64_t* geo_out,
                           float* mask_out, float* X_out, float* model_out, uint32_t* codes_out, char* kernel_out,
                           int32_t kernel_cap, char* nyquist_out, int32_t nyquist_cap, int64_t* launch_out) {
    if (!c || !V || !geo_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (kind < 0 || kind > 2) return fail(REPET_ERR_BAD_ARG, "kind: 0 period, 1 adaptive, 2 sim");
    if (B < 1 || C < 1 || C > 64 || T < 1 || F < 1 || cutoff < 0) return fail(REPET_ERR_BAD_ARG, "bad size");
    const int FS = (int)round_up(F, kFreqAlign);
    const int64_t Tpad = round_up(T, kTile), n_rows = Tpad + kPadRows, chan_stride = n_rows * FS, batch_stride = (int64_t)C * chan_stride;
    const int64_t model_rows = T / 3 + 2;
    if (chan_stride * 8 >= ((int64_t)1 << 31) || (int64_t)B * batch_stride > ((int64_t)1 << 27)) return fail(REPET_ERR_LIMIT, "too many cells for a stage test");
    const int64_t geo[8] = {Tpad, n_rows, FS, chan_stride, model_rows, 0, 0, 0};
    std::memcpy(geo_out, geo, sizeof(geo));
    if (!(want & 7) || (want & ~7)) return fail(REPET_ERR_BAD_ARG, "want: 1 mask plane, 2 X in place, 4 model");
    if ((want & 4) && (kind != 0 || (want & 3))) return fail(REPET_ERR_BAD_ARG, "the model is the period family's, and comes alone");
    if (((want & 1) && !mask_out) || ((want & 2) && (!X || !X_out)) || ((want & 4) && !model_out)) return fail(REPET_ERR_BAD_ARG, "null output");
    if (kind == 0) {
        if (periods) {
            if (min_period < 1) return fail(REPET_ERR_BAD_ARG, "min_period must be >= 1");
            for (int b = 0; b < B; ++b)
                if (periods[b] < min_period || periods[b] > model_rows) return fail(REPET_ERR_BAD_ARG, "a period outside [min_period, T / 3 + 2]");
        } else if (period_host < 1 || period_host > T || ((want & 4) && period_host > model_rows))
            return fail(REPET_ERR_BAD_ARG, "period must be in [1, T] (with a model: [1, T / 3 + 2])");
    } else if (kind == 1) {
        if (!periods || order < 1 || order > 1024) return fail(REPET_ERR_BAD_ARG, "adaptive: periods and an order in [1, 1024]");
        if (B != 1) return fail(REPET_ERR_BAD_ARG, "adaptive: one clip");
        for (int64_t t = 0; t < T; ++t)
            if (periods[t] < 1 || periods[t] > (1 << 20)) return fail(REPET_ERR_BAD_ARG, "a period outside [1, 2^20]");
    } else {
        if (!idx || !cnt) return fail(REPET_ERR_BAD_ARG, "null argument");
        if (width < 1 || max_count < 1 || max_count > width || idx_pitch < kMinIdxPitch || idx_pitch < width || idx_pitch > (1 << 16))
            return fail(REPET_ERR_BAD_ARG, "sim: 1 <= max_count <= width <= idx_pitch, idx_pitch >= 128");
        if (first_frame < 0 || first_frame > T || rows < 1 || rows < T - first_frame || rows > T)
            return fail(REPET_ERR_BAD_ARG, "sim: first_frame in [0, T], max(1, T - first_frame) <= rows <= T");
        if (frame_end == 0) frame_end = T;
        if (frame0 < 0 || frame0 > frame_end || frame_end > T) return fail(REPET_ERR_BAD_ARG, "sim: 0 <= frame0 <= frame_end <= T");
        if (parts < 1 || parts > 3) return fail(REPET_ERR_BAD_ARG, "parts: 1 main bins, 2 Nyquist bin, 3 both");
        if (median_path < 0 || median_path > 3) return fail(REPET_ERR_BAD_ARG, "median_path: 0 floats, 1 packed rank codes, 2 bit-sliced, 3 bit-sliced with the Nyquist column");
        if (median_path == 3 && (cutoff < 1 || parts != 1))
            return fail(REPET_ERR_BAD_ARG, "median_path 3: the Nyquist bin takes the column of bin 1, which needs cutoff >= 1, and parts = 1");
        for (int64_t k = 0; k < (int64_t)B * rows; ++k)
            if (cnt[k] < 0 || cnt[k] > max_count) return fail(REPET_ERR_BAD_ARG, "a list length outside [0, max_count]");
        for (int64_t k = 0; k < (int64_t)B * rows * width; ++k)
            if (idx[k] < 0 || idx[k] >= T) return fail(REPET_ERR_BAD_ARG, "a list entry outside [0, T)");
        if (median_path > 0) {
            if (B != 1 || first_frame != 0 || slot_start) return fail(REPET_ERR_BAD_ARG, "the rank paths take one clip from frame 0");
            if (F <= 128 || ((F - 1) & 127) || !rank_columns_supported(T) || max_count < 2 || max_count > 128)
                return fail(REPET_ERR_LIMIT, "rank-domain median: 1024 < n_frames <= 30720, n_freq - 1 a multiple of 128, lists of 2..128 entries");
            if (median_path >= 2 && !mask_sim_bits_supported(T, C, F - 1, max_count))
                return fail(REPET_ERR_LIMIT, "bit-sliced selection: at most 32 blocks of 64 bins over all channels, a power of two per channel");
            if (median_path >= 2 && !codes_out) return fail(REPET_ERR_BAD_ARG, "null output");
        }
    }
    DeviceGuard guard(c->device);
    const size_t planes = (size_t)B * C, cells = planes * chan_stride;
    const int fill = prefill & 255;
    Scratch Vd, Xd, Md, Wd, Pd, Id, Nd, Sd, Rd, Vsd, RCd, CPd, MCd;
    HIP_TRY(Vd.b.ensure(cells * sizeof(float)));
    HIP_TRY(hipMemsetAsync(Vd.b.p, fill, cells * sizeof(float), c->stream));
    for (size_t p = 0; p < planes; ++p)
        HIP_TRY(hipMemcpy2DAsync(Vd.b.as<float>() + p * chan_stride, (size_t)FS * sizeof(float), V + p * (size_t)T * F, (size_t)F * sizeof(float),
                                 (size_t)F * sizeof(float), T, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_fill_pad_rows(Vd.b.as<float>(), chan_stride, (int32_t)planes, Tpad, FS, c->stream));
    if (want & 2) {
        HIP_TRY(Xd.b.ensure(cells * sizeof(float2)));
        HIP_TRY(hipMemsetAsync(Xd.b.p, fill, cells * sizeof(float2), c->stream));
        for (size_t p = 0; p < planes; ++p)
            HIP_TRY(hipMemcpy2DAsync(Xd.b.as<float2>() + p * chan_stride, (size_t)FS * sizeof(float2), X + p * (size_t)T * F * 2,
                                     (size_t)F * sizeof(float2), (size_t)F * sizeof(float2), T, hipMemcpyHostToDevice, c->stream));
    }
    if (want & 1) {
        HIP_TRY(Md.b.ensure(cells * sizeof(float)));
        HIP_TRY(hipMemsetAsync(Md.b.p, fill, cells * sizeof(float), c->stream));
    }
    const size_t model_cells = planes * model_rows * FS;
    if (want & 4) {
        HIP_TRY(Wd.b.ensure(model_cells * sizeof(float)));
        HIP_TRY(hipMemsetAsync(Wd.b.p, fill, model_cells * sizeof(float), c->stream));
    }
    MaskArgs m{};
    m.V = Vd.b.as<float>(); m.chan_stride = chan_stride; m.n_channels = C; m.T = T; m.F = F; m.FS = FS;
    m.X = (want & 2) ? Xd.b.as<float2>() : nullptr; m.mask = (want & 1) ? Md.b.as<float>() : nullptr;
    m.cutoff = cutoff; m.pad_row = Tpad; m.n_batch = B; m.batch_stride = batch_stride;
    if (want & 4) { m.model = Wd.b.as<float>(); m.model_batch_stride = (int64_t)C * model_rows * FS; m.model_chan_stride = model_rows * FS; }
    MaskLaunch info;
    bool from_codes = false;
    if (kind == 0) {
        if (periods) {
            HIP_TRY(Pd.b.ensure((size_t)B * sizeof(int32_t)));
            HIP_TRY(hipMemcpyAsync(Pd.b.p, periods, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(launch_mask_period(m, Pd.b.as<int32_t>(), 0, min_period, c->stream, &info));
        } else
            HIP_TRY(launch_mask_period(m, nullptr, period_host, period_host, c->stream, &info));
    } else if (kind == 1) {
        HIP_TRY(Pd.b.ensure((size_t)T * sizeof(int32_t)));
        HIP_TRY(hipMemcpyAsync(Pd.b.p, periods, (size_t)T * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(launch_mask_adaptive(m, Pd.b.as<int32_t>(), order, c->stream, &info));
    } else {
        const size_t list_rows = (size_t)B * rows;
        HIP_TRY(Id.b.ensure(list_rows * idx_pitch * sizeof(int32_t)));
        HIP_TRY(Nd.b.ensure(list_rows * sizeof(int32_t)));
        HIP_TRY(hipMemsetAsync(Id.b.p, 0, list_rows * idx_pitch * sizeof(int32_t), c->stream));
        HIP_TRY(hipMemcpy2DAsync(Id.b.p, (size_t)idx_pitch * sizeof(int32_t), idx, (size_t)width * sizeof(int32_t), (size_t)width * sizeof(int32_t),
                                 list_rows, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(Nd.b.p, cnt, list_rows * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        m.idx_batch_stride = rows * idx_pitch; m.cnt_batch_stride = rows; m.frame0 = frame0; m.frame_end = frame_end;
        if (slot_start) {
            HIP_TRY(Sd.b.ensure((size_t)B * sizeof(int64_t)));
            HIP_TRY(hipMemcpyAsync(Sd.b.p, slot_start, (size_t)B * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
            m.slot_start = Sd.b.as<int64_t>(); m.slot_bias = slot_bias;
        }
        if (median_path > 0) {                               // run_rank_columns' calls, the path forced instead of read from the environment
            const int n_cols = F - 1;
            const int64_t vs_pitch = round_up(T, 32);
            const bool bits = median_path >= 2;
            HIP_TRY(Vsd.b.ensure((size_t)C * n_cols * vs_pitch * sizeof(float)));
            HIP_TRY(RCd.b.ensure((size_t)C * n_cols * vs_pitch * sizeof(unsigned short)));
            RankArgs a{};
            a.V = Vd.b.as<float>(); a.chan_stride = chan_stride; a.n_channels = C; a.T = T; a.FS = FS; a.n_cols = n_cols;
            a.r_chan_stride = chan_stride; a.Vs = Vsd.b.as<float>(); a.vs_pitch = vs_pitch; a.codes = RCd.b.as<unsigned short>();
            if (bits) {
                a.n_planes = code_planes_for(T);
                HIP_TRY(CPd.b.ensure((size_t)T * a.n_planes * 64 * sizeof(unsigned)));
                HIP_TRY(hipMemsetAsync(CPd.b.p, 0, (size_t)T * a.n_planes * 64 * sizeof(unsigned), c->stream));
                a.P = CPd.b.as<unsigned>();
                HIP_TRY(MCd.b.ensure((size_t)C * chan_stride * sizeof(unsigned)));
                HIP_TRY(hipMemsetAsync(MCd.b.p, fill, (size_t)C * chan_stride * sizeof(unsigned), c->stream));
                m.median_codes = MCd.b.as<unsigned>();
                if (median_path == 3) { a.swap_col = m.swap_col = 1; a.swap_bin = m.swap_bin = F - 1; }
            } else {
                HIP_TRY(Rd.b.ensure((size_t)C * chan_stride * sizeof(unsigned short)));
                HIP_TRY(hipMemsetAsync(Rd.b.p, 0, (size_t)C * chan_stride * sizeof(unsigned short), c->stream));
                HIP_TRY(launch_fill_rank_pad_rows(Rd.b.as<unsigned short>(), chan_stride, C, Tpad, FS, c->stream));
                a.R = Rd.b.as<unsigned short>();
            }
            HIP_TRY(launch_rank_columns(a, c->stream));
            m.R = a.R; m.r_chan_stride = a.r_chan_stride; m.Vs = a.Vs; m.vs_pitch = vs_pitch; m.n_rank_cols = n_cols;
            m.P = a.P; m.n_planes = a.n_planes;
        }
        // (as exec_sim: the lookups of the bit-sliced selection are the caller's launch)
        HIP_TRY(launch_mask_sim(m, Id.b.as<int32_t>(), idx_pitch, Nd.b.as<int32_t>(), first_frame, max_count, c->stream, parts, m.P != nullptr, &info));
        if (median_path > 0 && (parts & 1) && frame_end > frame0) {
            const char* expect = median_path >= 2 ? "mask_sim_bits_kernel" : "mask_sim_rank_kernel";
            if (std::strcmp(info.kernel, expect) != 0) {
                (void)hipStreamSynchronize(c->stream);
                return fail(REPET_ERR_LIMIT, "the launcher did not take the median path asked for");
            }
            if (median_path >= 2) { HIP_TRY(launch_mask_from_codes(m, Nd.b.as<int32_t>(), c->stream)); from_codes = true; }
        }
    }
    if (want & 1) HIP_TRY(hipMemcpyAsync(mask_out, Md.b.p, cells * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (want & 2) HIP_TRY(hipMemcpyAsync(X_out, Xd.b.p, cells * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
    if (want & 4) HIP_TRY(hipMemcpyAsync(model_out, Wd.b.p, model_cells * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (kind == 2 && median_path >= 2)
        HIP_TRY(hipMemcpyAsync(codes_out, MCd.b.p, (size_t)C * chan_stride * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    auto put = [](char* out, int32_t cap, const char* name) {
        if (out && cap > 0) { std::strncpy(out, name, (size_t)cap - 1); out[cap - 1] = 0; }
    };
    put(kernel_out, kernel_cap, info.kernel);
    put(nyquist_out, nyquist_cap, info.nyquist);
    if (launch_out) {
        const int64_t v[16] = {info.net, info.flag, info.parts, info.grid[0], info.grid[1], info.grid[2], info.nyquist_net, info.nyquist_preload,
                               info.nyquist_grid[0], info.nyquist_grid[1], info.nyquist_grid[2], from_codes, 0, 0, 0, 0};
        std::memcpy(launch_out, v, sizeof(v));
    }
    return REPET_OK;
}

int repet_rank_columns(repet_ctx* c, const float* v, int64_t T, int32_t F, uint16_t* codes_out, float* sorted_out) {
    if (!c || !v || !codes_out || !sorted_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (F < 128) return fail(REPET_ERR_BAD_ARG, "needs at least 128 bins");
    if (!rank_columns_supported(T)) return fail(REPET_ERR_LIMIT, "rank transform: 1024 < n_frames <= 30720");
    DeviceGuard guard(c->device);
    const int FS = (int)round_up(F, kFreqAlign), n_cols = F & ~127;
    const int64_t rows = T + kPadRows, vs_pitch = round_up(T, 32);
    RP_TRY(stage_matrix_in(c, c->V, v, T, F, FS, rows));
    HIP_TRY(c->R.ensure((size_t)rows * FS * sizeof(unsigned short)));
    c->r_pads_ptr = nullptr;                              // this export lays R out differently
    HIP_TRY(c->Vs.ensure((size_t)n_cols * vs_pitch * sizeof(float)));
    RankArgs a{};
    a.V = c->V.as<float>(); a.chan_stride = rows * FS; a.n_channels = 1; a.T = T; a.FS = FS; a.n_cols = n_cols;
    a.R = c->R.as<unsigned short>(); a.r_chan_stride = rows * FS; a.Vs = c->Vs.as<float>(); a.vs_pitch = vs_pitch;
    HIP_TRY(c->rank_codes.ensure((size_t)n_cols * vs_pitch * sizeof(unsigned short)));
    a.codes = c->rank_codes.as<unsigned short>();
    HIP_TRY(launch_rank_columns(a, c->stream));
    HIP_TRY(hipMemcpy2DAsync(codes_out, (size_t)n_cols * sizeof(uint16_t), c->R.p, (size_t)FS * sizeof(uint16_t),
                             (size_t)n_cols * sizeof(uint16_t), T, hipMemcpyDeviceToHost, c->stream));
    return d2h_pitched(c, sorted_out, c->Vs.as<float>(), vs_pitch, n_cols, T);
}

int repet_ctx_download_input(repet_ctx* c, float* samples_out, float* remainders_out, int32_t* has_remainders) {
    if (!c || !samples_out || !remainders_out || !has_remainders) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (c->n_channels < 1) return fail(REPET_ERR_BAD_ARG, "no clip uploaded");
    DeviceGuard guard(c->device);
    const size_t bytes = (size_t)c->n_samples * c->n_channels * c->n_clips * sizeof(float);
    if (c->has_lo && c->ring.lo_in_flight) HIP_TRY(hipStreamWaitEvent(c->stream, c->ring.lo_done, 0));
    HIP_TRY(hipMemcpyAsync(samples_out, c->audio.p, bytes, hipMemcpyDeviceToHost, c->stream));
    if (c->has_lo) HIP_TRY(hipMemcpyAsync(remainders_out, c->audio_lo.p, bytes, hipMemcpyDeviceToHost, c->stream));
    else std::memset(remainders_out, 0, bytes);
    HIP_TRY(hipStreamSynchronize(c->stream));
    *has_remainders = c->has_lo ? 1 : 0;
    return REPET_OK;
}

int repet_ctx_last_periods(repet_ctx* c, int32_t* out, int32_t capacity, int32_t* n_written) {
    if (!c || !out || !n_written) return fail(REPET_ERR_BAD_ARG, "null argument");
    DeviceGuard guard(c->device);
    const int n = std::min(capacity, c->last_n_periods);
    if (n > 0) HIP_TRY(hipMemcpy(out, c->periods.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    *n_written = n;
    return REPET_OK;
}

int repet_ctx_last_sim_indices(repet_ctx* c, int32_t* idx_out, int32_t* count_out, int32_t n_rows, int32_t number) {
    if (!c || !idx_out || !count_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    // a batch context holds the lists of its clips back to back: n_rows may be rows-per-clip (first clip) or all of them
    if ((n_rows != c->last_idx_rows && n_rows != c->last_idx_rows * c->last_idx_batch) || number != c->last_idx_number)
        return fail(REPET_ERR_BAD_ARG, "shape does not match the last run");
    DeviceGuard guard(c->device);
    if (n_rows > 0) {
        HIP_TRY(hipMemcpy2D(idx_out, (size_t)number * sizeof(int32_t), c->idx.p, (size_t)c->last_idx_pitch * sizeof(int32_t),
                            (size_t)number * sizeof(int32_t), n_rows, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(count_out, c->cnt.p, (size_t)n_rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return REPET_OK;
}

int repet_ctx_last_sim_indices_clip(repet_ctx* c, int32_t clip, int32_t* idx_out, int32_t* count_out, int32_t n_rows, int32_t number) {
    if (!c || !idx_out || !count_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    // (clip 0 takes what repet_ctx_last_sim_indices takes: the rows of one clip, or of all clips back to back)
    const bool all = clip == 0 && n_rows == c->last_idx_rows * c->last_idx_batch;
    if ((n_rows != c->last_idx_rows && !all) || number != c->last_idx_number) return fail(REPET_ERR_BAD_ARG, "shape does not match the last run");
    if (clip < 0 || clip >= c->last_idx_batch) return fail(REPET_ERR_BAD_ARG, "the last run kept no lists of that clip");
    DeviceGuard guard(c->device);
    HIP_TRY(hipStreamSynchronize(c->stream));               // (behind a run that was only enqueued)
    if (n_rows > 0) {
        HIP_TRY(hipMemcpy2D(idx_out, (size_t)number * sizeof(int32_t), c->idx.as<int32_t>() + (size_t)clip * c->last_idx_rows * c->last_idx_pitch,
                            (size_t)c->last_idx_pitch * sizeof(int32_t), (size_t)number * sizeof(int32_t), n_rows, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(count_out, c->cnt.as<int32_t>() + (size_t)clip * c->last_idx_rows, (size_t)n_rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return REPET_OK;
}

int repet_ctx_last_clip_passes(repet_ctx* c, int32_t* passes) {
    if (!c || !passes) return fail(REPET_ERR_BAD_ARG, "null argument");
    *passes = c->last_clip_passes;
    return REPET_OK;
}

int repet_ctx_last_median_codes(repet_ctx* c, uint32_t* out, int64_t n_frames, int32_t n_bins) {
    if (!c || !out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (c->last_median_path != 2 || !c->median_codes.p) return fail(REPET_ERR_BAD_ARG, "the last run did not take the bit-sliced selection");
    if (n_frames != c->last_T || n_bins < 1 || n_bins > c->last_FS) return fail(REPET_ERR_BAD_ARG, "shape does not match the last run");
    DeviceGuard guard(c->device);
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int ch = 0; ch < c->n_channels; ++ch)
        HIP_TRY(hipMemcpy2D(out + (size_t)ch * n_frames * n_bins, (size_t)n_bins * 4, c->median_codes.as<unsigned>() + (size_t)ch * c->last_chan_stride,
                            (size_t)c->last_FS * 4, (size_t)n_bins * 4, n_frames, hipMemcpyDeviceToHost));
    return REPET_OK;
}

int repet_ctx_last_median_path(repet_ctx* c, int32_t* path) {
    if (!c || !path) return fail(REPET_ERR_BAD_ARG, "null argument");
    *path = c->last_median_path;
    return REPET_OK;
}

int repet_ctx_last_frame_count(repet_ctx* c, int64_t* n_frames) {
    if (!c || !n_frames) return fail(REPET_ERR_BAD_ARG, "null argument");
    *n_frames = c->last_T;
    return REPET_OK;
}

// the counters of the last run, the copies of every diagnostic counter added up ([8] is a maximum) -- common.h, kStatShards
static int read_stats(repet_ctx* c, unsigned int (&total)[kRefineStats]) {
    std::vector<unsigned int> words(kStatWords);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(words.data(), c->refine_stats.p, kStatWords * sizeof(unsigned int), hipMemcpyDeviceToHost));
    for (int k = 0; k < kRefineStats; ++k) total[k] = words[k];
    for (int sh = 1; sh <= kStatShards; ++sh)
        for (int k = 0; k < kRefineStats; ++k)
            total[k] = (k == 8) ? std::max(total[k], words[sh * kRefineStats + k]) : total[k] + words[sh * kRefineStats + k];
    return REPET_OK;
}

int repet_ctx_last_exact_stats(repet_ctx* c, int64_t out[8]) {
    if (!c || !out) return fail(REPET_ERR_BAD_ARG, "null argument");
    for (int k = 0; k < 8; ++k) out[k] = 0;
    out[5] = c->has_lo ? 1 : 0;
    if (!c->refine_stats.p) return REPET_OK;
    DeviceGuard guard(c->device);
    unsigned int host[kRefineStats] = {};
    RP_TRY(read_stats(c, host));
    out[0] = host[4] + host[12] - host[14]; out[1] = host[6]; out[2] = host[7]; out[3] = host[8]; out[4] = host[9];
    out[6] = host[12]; out[7] = host[14];
    return REPET_OK;
}

#ifdef REPET_EXACT_STAMPS
int repet_debug_exact_phases(repet_ctx* c, int64_t out[6]) {
    unsigned int host[kRefineStats] = {};
    RP_TRY(read_stats(c, host));
    for (int k = 0; k < 6; ++k) out[k] = host[24 + k];
    return REPET_OK;
}
#endif

int repet_ctx_last_refine_stats(repet_ctx* c, int64_t out[4]) {
    if (!c || !out) return fail(REPET_ERR_BAD_ARG, "null argument");
    for (int k = 0; k < 4; ++k) out[k] = 0;
    if (!c->refine_stats.p) return REPET_OK;
    DeviceGuard guard(c->device);
    unsigned int host[kRefineStats] = {};
    RP_TRY(read_stats(c, host));
    for (int k = 0; k < 4; ++k) out[k] = host[k];
    return REPET_OK;
}

// ---- stage entry of the production peak-picking launchers (tests/test_gpu_peaks_stages.py) -----------------------------
// repet_local_maxima above is launch_local_maxima in mode 0 without refinement, batch, origin, shift or scratch: no pipeline
// launches the kernels that way. This one runs the chain of exec_sim / exec_simonline / the live handles -- launch_segment_maxima
// where local_maxima_segments_apply says so, make_refine, launch_local_maxima, run_exact_rows -- on buffers the caller lays out:
//   M     (n_batch, m_rows, n_cols) fp32, copied to rows of `pitch` floats (mode 0: matrix rows; modes 1 and 2: the band as
//         run_gram_band lays it out, band row = frame - shift)
//   unit  (n_batch, n_frames, F) fp32 unit rows, copied to pitch FS = round_up(F, 32) with zero pad bins (PeakRefine::unit_rows;
//         mode 0: row = frame = column; modes 1 and 2: row = band row)
//   hi, lo (nullable) (n_batch, n_samples, C) fp32: the ExactSource; frame row fr starts at sample frame_sample0 + fr * W / 2
//   refine 0: none (unit, hi unused); 1: level 1 only (make_refine with no rows for the second level); 2: both levels
//   origin (nullable, n_batch) and start: PeakBatch; the batch is passed when n_batch > 1, origin is given or start > 0
// idx, count, the float64 unit-row table and every cell of the device copy of M the caller did not supply hold the byte
// `prefill` before the launch. Every row the launch can touch is walked on the host first, with the cells it may read: a
// band row or unit row outside the buffers is REPET_ERR_BAD_ARG, never an out-of-range load.
// Out: idx (n_batch, n_rows + 1, KP) and count (n_batch, n_rows + 1) whole (the last row of a clip is a guard no launch owns),
// stats[32] the counters added up ([8] a maximum), delta[2] = delta, delta2 of the launch, u64 (n_batch, n_frames, FS) and
// stamped (n_batch, n_frames; 1: the row's stamp is this launch's generation) when refine == 2, family (PeakLaunch),
// launch[8] = QMAX, RD, unit_rows_f64_wg_kernel variant, lite relaunch, FFT plan of local_maxima_exact_kernel, KP, FS, 0.
int repet_debug_peaks_stage(repet_ctx* c, const float* M, int32_t n_batch, int64_t m_rows, int32_t n_cols, int64_t pitch,
                            const float* unit, int64_t n_frames, int32_t F, const float* hi, const float* lo, int64_t n_samples,
                            int32_t C, int32_t W, int64_t frame_sample0, int32_t mode, int64_t row0, int64_t n_rows, double min_value,
                            int32_t d, int32_t number, int64_t shift, const int64_t* origin, int32_t start, int32_t with_scratch,
                            int32_t refine, int32_t prefill, int32_t* idx_out, int32_t* count_out, int64_t* stats_out,
                            double* delta_out, double* u64_out, int32_t* stamped_out, char* family_out, int32_t family_cap,
                            int64_t* launch_out) {
    if (!c || !M || !idx_out || !count_out || !stats_out || !delta_out || !launch_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (mode < 0 || mode > 2 || refine < 0 || refine > 2) return fail(REPET_ERR_BAD_ARG, "mode in 0..2, refine in 0..2");
    if (n_batch < 1 || n_batch > 64 || m_rows < 1 || n_cols < 1 || pitch < n_cols || pitch > (1 << 20) || n_rows < 1 || row0 < 0 || d < 0 ||
        number < 1 || number > (1 << 16) || row0 + n_rows > ((int64_t)1 << 30))
        return fail(REPET_ERR_BAD_ARG, "bad size");
    if ((int64_t)n_batch * m_rows * pitch > ((int64_t)1 << 27)) return fail(REPET_ERR_LIMIT, "too many cells for a stage test");
    const int FS = refine ? (int)round_up(F, kFreqAlign) : 0;
    if (refine) {
        if (!unit || n_frames < 1 || F < 1 || (int64_t)n_batch * n_frames * FS > ((int64_t)1 << 27)) return fail(REPET_ERR_BAD_ARG, "refinement: unit rows");
    }
    if (refine == 2) {
        if (!hi || !u64_out || !stamped_out || n_samples < 1 || C < 1 || C > 64 || W < 64 || W > 8192 || (W & (W - 1)) || F != W / 2 + 1 ||
            (int64_t)n_batch * n_samples * C > ((int64_t)1 << 27) || frame_sample0 < -(int64_t)W || frame_sample0 > n_samples)
            return fail(REPET_ERR_BAD_ARG, "second level: audio (n_batch, n_samples, C), W a power of two, F = W / 2 + 1");
    }
    if (mode == 0) {
        if (origin || start != 0 || shift != 0) return fail(REPET_ERR_BAD_ARG, "mode 0 takes no origin, start or shift");
        if (row0 + n_rows > m_rows) return fail(REPET_ERR_BAD_ARG, "mode 0: rows outside the matrix");
        if (refine && n_frames < std::max<int64_t>(n_cols, row0 + n_rows)) return fail(REPET_ERR_BAD_ARG, "mode 0: a unit row per row and column");
    } else {
        if (start < 0 || start > n_cols) return fail(REPET_ERR_BAD_ARG, "start in [0, n_cols]");
        const int64_t first_active = (start > 0 ? start : n_cols) - 1;
        for (int b = 0; b < n_batch; ++b) {
            const int64_t o = origin ? origin[b] : 0;
            if (o < -((int64_t)1 << 61) || o > ((int64_t)1 << 61)) return fail(REPET_ERR_BAD_ARG, "origin out of range");
            for (int64_t r = 0; r < n_rows; ++r) {
                const int64_t jl = row0 + r - o;                      // the row counted from the clip's own first frame
                if (origin && jl < first_active) continue;             // inactive: no list, nothing read
                if (jl < 0) return fail(REPET_ERR_BAD_ARG, "a row before the clip's first frame");
                const int64_t cols = std::min<int64_t>(n_cols, jl + 1), top = row0 + r - shift, bottom = top - (cols - 1);
                if (bottom < 0 || top >= m_rows || (refine && top >= n_frames)) return fail(REPET_ERR_BAD_ARG, "a band row outside the band");
            }
        }
    }
    DeviceGuard guard(c->device);
    const int fill = prefill & 255;
    const int KP = std::max(number, kMinIdxPitch);
    const int64_t rows_alloc = n_rows + 1;
    const size_t m_cells = (size_t)n_batch * m_rows * pitch + 4096;     // (slack behind the last row for 16-byte loads up to the pitch)
    Scratch Md, Ud, Hd, Ld, Id, Nd, Od, Sd, Pd;
    HIP_TRY(Md.b.ensure(m_cells * sizeof(float)));
    HIP_TRY(hipMemsetAsync(Md.b.p, fill, m_cells * sizeof(float), c->stream));
    HIP_TRY(hipMemcpy2DAsync(Md.b.p, (size_t)pitch * sizeof(float), M, (size_t)n_cols * sizeof(float), (size_t)n_cols * sizeof(float),
                             (size_t)n_batch * m_rows, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(Id.b.ensure((size_t)n_batch * rows_alloc * KP * sizeof(int32_t)));
    HIP_TRY(Nd.b.ensure((size_t)n_batch * rows_alloc * sizeof(int32_t)));
    HIP_TRY(hipMemsetAsync(Id.b.p, fill, (size_t)n_batch * rows_alloc * KP * sizeof(int32_t), c->stream));
    HIP_TRY(hipMemsetAsync(Nd.b.p, fill, (size_t)n_batch * rows_alloc * sizeof(int32_t), c->stream));
    if (refine) {
        const size_t u_cells = (size_t)n_batch * n_frames * FS;
        HIP_TRY(Ud.b.ensure(u_cells * sizeof(float)));
        HIP_TRY(hipMemsetAsync(Ud.b.p, 0, u_cells * sizeof(float), c->stream));
        HIP_TRY(hipMemcpy2DAsync(Ud.b.p, (size_t)FS * sizeof(float), unit, (size_t)F * sizeof(float), (size_t)F * sizeof(float),
                                 (size_t)n_batch * n_frames, hipMemcpyHostToDevice, c->stream));
    }
    Tables* tb = nullptr;
    if (refine == 2) {
        const size_t a_bytes = (size_t)n_batch * n_samples * C * sizeof(float);
        RP_TRY(get_tables(c, W, &tb));
        HIP_TRY(Hd.b.ensure(a_bytes));
        HIP_TRY(hipMemcpyAsync(Hd.b.p, hi, a_bytes, hipMemcpyHostToDevice, c->stream));
        if (lo) {
            HIP_TRY(Ld.b.ensure(a_bytes));
            HIP_TRY(hipMemcpyAsync(Ld.b.p, lo, a_bytes, hipMemcpyHostToDevice, c->stream));
        }
        HIP_TRY(c->u64.ensure((size_t)n_batch * n_frames * FS * sizeof(double)));
        HIP_TRY(hipMemsetAsync(c->u64.p, fill, (size_t)n_batch * n_frames * FS * sizeof(double), c->stream));
    }
    if (origin) {
        HIP_TRY(Od.b.ensure((size_t)n_batch * sizeof(int64_t)));
        HIP_TRY(hipMemcpyAsync(Od.b.p, origin, (size_t)n_batch * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    }
    float* seg = nullptr;
    const int seg_pitch = segment_pitch((int)pitch);
    if (local_maxima_segments_apply(n_cols, d, pitch, mode, n_batch)) {                  // as exec_sim: records of every row of M
        HIP_TRY(Sd.b.ensure((size_t)m_rows * 3 * seg_pitch * sizeof(float)));
        HIP_TRY(hipMemsetAsync(Sd.b.p, fill, (size_t)m_rows * 3 * seg_pitch * sizeof(float), c->stream));
        seg = Sd.b.as<float>();
        HIP_TRY(launch_segment_maxima(Md.b.as<float>(), m_rows, n_cols, pitch, seg, seg_pitch, c->stream));
    }
    PeakRefine rf{};
    if (refine)
        RP_TRY(make_refine(c, Ud.b.as<float>(), FS, min_value, &rf, refine == 2 ? n_rows : 0, n_batch, n_cols, d, refine == 2 ? n_frames : 0));
    const PeakBatch pb{n_batch, m_rows * pitch, rows_alloc * KP, rows_alloc, n_frames * (int64_t)FS, origin ? Od.b.as<int64_t>() : nullptr, start};
    const PeakBatch* batch = (n_batch > 1 || origin || start > 0) ? &pb : nullptr;
    void* scratch = nullptr;
    if (with_scratch) {
        const size_t bytes = local_maxima_scratch_bytes(n_rows, n_cols, d);
        if (bytes > 0) { HIP_TRY(Pd.b.ensure(bytes)); HIP_TRY(hipMemsetAsync(Pd.b.p, fill, bytes, c->stream)); scratch = Pd.b.p; }
    }
    PeakLaunch info;
    hipError_t e = launch_local_maxima(Md.b.as<float>(), n_rows, row0, n_cols, pitch, mode, (float)min_value, d, number, Id.b.as<int32_t>(), KP,
                                       Nd.b.as<int32_t>(), c->stream, shift, refine ? &rf : nullptr, batch, scratch, nullptr, seg, seg_pitch, &info);
    if (e == hipErrorInvalidValue) { (void)hipStreamSynchronize(c->stream); return fail(REPET_ERR_LIMIT, "row too long for the peak-picking kernel"); }
    HIP_TRY(e);
    if (refine == 2) {
        const Geo g = make_geo(W, W / 2, n_frames, C);
        if (g.FS != FS || g.F != F) { (void)hipStreamSynchronize(c->stream); return fail(REPET_ERR_BAD_ARG, "F does not match W"); }
        RP_TRY(run_exact_rows(c, tb, g, Md.b.as<float>(), row0, n_cols, pitch, mode, (float)min_value, d, number, Id.b.as<int32_t>(), KP,
                              Nd.b.as<int32_t>(), shift, rf, batch, Hd.b.as<float>(), lo ? Ld.b.as<float>() : nullptr, n_samples,
                              n_samples * C, frame_sample0, n_frames, n_batch, &info));
    }
    HIP_TRY(hipMemcpyAsync(idx_out, Id.b.p, (size_t)n_batch * rows_alloc * KP * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(count_out, Nd.b.p, (size_t)n_batch * rows_alloc * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    for (int k = 0; k < kRefineStats; ++k) stats_out[k] = 0;
    if (refine) {
        unsigned int total[kRefineStats] = {};
        RP_TRY(read_stats(c, total));
        for (int k = 0; k < kRefineStats; ++k) stats_out[k] = total[k];
    }
    if (refine == 2 && rf.redo_list) {
        const size_t n_gen = (size_t)n_batch * n_frames;
        std::vector<unsigned int> gens(n_gen);
        HIP_TRY(hipMemcpyAsync(u64_out, c->u64.p, n_gen * FS * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(gens.data(), c->u64_gen.p, n_gen * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (size_t k = 0; k < n_gen; ++k) stamped_out[k] = gens[k] == rf.gen ? 1 : 0;
    } else if (refine == 2)
        return fail(REPET_ERR_LIMIT, "the second level is switched off");
    HIP_TRY(hipStreamSynchronize(c->stream));
    delta_out[0] = rf.delta; delta_out[1] = rf.delta2;
    if (family_out && family_cap > 0) { std::strncpy(family_out, info.family, (size_t)family_cap - 1); family_out[family_cap - 1] = 0; }
    const int64_t v[8] = {info.qmax, info.rd, info.unit_kq, info.lite, info.exact_fft, KP, FS, 0};
    std::memcpy(launch_out, v, sizeof(v));
    return REPET_OK;
}

}  // extern "C"

// ---- the stage entry of devio.hip (tests/test_gpu_devio_stages.py) ------------------------------------------------------
// repet_debug_devio_stage runs ONE production launcher of devio.hip, unchanged, on device buffers the caller describes ("arenas").
// Arena k is arena_bytes[k] bytes of the caller's; it is uploaded into an allocation of its own whose every other byte holds
// `prefill`, its first byte arena_shift[k] (0, 4, 8 or 12; 2 for an arena of 16-bit elements) bytes behind a 256-byte boundary, and it comes back whole with
// kArenaGuard bytes of that prefill in front of and behind it (arena_out[k]: arena_bytes[k] + 2 * kArenaGuard bytes). Every pointer
// argument of a launcher is a pair of words (arena, offset in elements of the pointer's type; arena < 0: null). The words `iv`
// are read in the order the op's branch below reads them; `fv` holds the float arguments. Before anything is enqueued the entry
// walks what the launch may read and write: a cell outside the caller's bytes of an arena is REPET_ERR_BAD_ARG, never an access.
// report_out[24] is the launcher's DevioReport: launches, grid[3], dense[2], src_vec[5], dst_vec[5], held_vec[5], 0 ..
namespace {
constexpr int64_t kArenaGuard = 512;
constexpr int64_t kStageMax = (int64_t)1 << 28;

struct Ref { int64_t arena = -1, off = 0; };

struct Words {
    const int64_t* v; int32_t n; int32_t at = 0; bool bad = false;
    int64_t any() { if (at >= n) { bad = true; return 0; } return v[at++]; }
    int64_t size() { const int64_t x = any(); if (x < 0 || x > kStageMax) bad = true; return bad ? 0 : x; }        // a count or a stride
    int64_t off() { const int64_t x = any(); if (x < -kStageMax || x > kStageMax) bad = true; return bad ? 0 : x; }
    // the length of a list that follows in the words: never more than the words that are left (it sizes a host vector)
    int64_t count() { const int64_t x = size(); if (x > n - at) bad = true; return bad ? 0 : x; }
    Ref ref() { Ref r; r.arena = off(); r.off = size(); return r; }
};

struct Arenas {
    std::vector<Scratch> dev; std::vector<char*> first; std::vector<int64_t> bytes; std::vector<const char*> host; std::vector<int32_t> shift;
    explicit Arenas(int n) : dev((size_t)n), first((size_t)n), bytes((size_t)n), host((size_t)n), shift((size_t)n) {}
    // elements [lo, hi) of `es` bytes, counted from the element r names, lie in the caller's bytes (nothing to hold: true).
    // An arena 2 bytes off the boundary holds 16-bit elements only: nothing wider is ever read at half its own alignment.
    bool holds(Ref r, int64_t lo, int64_t hi, int es) const {
        if (r.arena >= 0 && r.arena < (int64_t)bytes.size() && shift[(size_t)r.arena] == 2 && es != 2) return false;
        if (hi <= lo) return r.arena < (int64_t)bytes.size();
        if (r.arena < 0 || r.arena >= (int64_t)bytes.size()) return false;
        return r.off + lo >= 0 && (r.off + hi) * es <= bytes[(size_t)r.arena];
    }
    bool null_or_holds(Ref r, int64_t lo, int64_t hi, int es) const { return r.arena < 0 || holds(r, lo, hi, es); }
    template <typename T> T* at(Ref r) const { return r.arena < 0 ? nullptr : reinterpret_cast<T*>(first[(size_t)r.arena] + r.off * (int64_t)sizeof(T)); }
    void* at_bytes(Ref r, int es) const { return r.arena < 0 ? nullptr : first[(size_t)r.arena] + r.off * es; }
    template <typename T> const T* on_host(Ref r) const { return reinterpret_cast<const T*>(host[(size_t)r.arena] + r.off * (int64_t)sizeof(T)); }
    bool aligned(Ref r, int es, int to) const { return r.arena < 0 || !(reinterpret_cast<uintptr_t>(at_bytes(r, es)) % (uintptr_t)to); }
};

// the elements of a [B][n][C] are few enough that no extent below overflows: at most kStageMax of them
bool plane_ok(int64_t B, int64_t n, int64_t C) {
    return B >= 1 && n >= 1 && C >= 1 && n * C <= kStageMax && B * (n * C) <= kStageMax;       // (each factor is at most kStageMax = 2^28)
}
// one past the largest element offset of a strided [B][n][C]
int64_t span3(const int64_t st[3], int64_t B, int64_t n, int64_t C) {
    return B < 1 || n < 1 || C < 1 ? 0 : st[0] * (B - 1) + st[1] * (n - 1) + st[2] * (C - 1) + 1;
}
// one past the last float of a part's runs over S streams (or slots)
int64_t run_span(int64_t len, int64_t blocks, int64_t block, int64_t S, int64_t stream) {
    return len < 1 || blocks < 1 || S < 1 ? 0 : (S - 1) * stream + (blocks - 1) * block + len;
}

enum DevioOp {
    kOpIngest = 0, kOpEgress, kOpEmit, kOpLevels, kOpTailClear, kOpAppend, kOpRowCopies, kOpSlideHeld, kOpSlotSet, kOpFeed, kOpTake,
    kOpSlotReset, kOpSlotExport, kOpSlotImport, kOpGainFill, kOpGainSet, kOpGainCommit, kOpBandExpand, kOpBandCommit
};

// the gain words of emit and levels: mode (0 none, 1 scalar fv[0], 2 tables), a_cur, a_tgt, ramp
bool read_gain(Words& w, const Arenas& A, int64_t S, const double* fv, int32_t n_fv, EmitGain& g, bool& present) {
    const int64_t mode = w.size();
    const Ref cur = w.ref(), tgt = w.ref();
    g.ramp = w.off();
    if (w.bad || mode > 2) return false;
    present = mode != 0;
    if (mode == 1) { if (n_fv < 1) return false; g.scalar = true; g.a = (float)fv[0]; }
    if (mode == 2) {
        if (!A.holds(tgt, 0, S, 4) || !A.null_or_holds(cur, 0, S, 4)) return false;
        g.a_cur = A.at<float>(cur); g.a_tgt = A.at<float>(tgt);
    }
    return true;
}

hipError_t run_devio_op(int32_t op, const Arenas& A, Words& w, const double* fv, int32_t n_fv, hipStream_t s, bool& refused) {
    refused = true;                                               // (every early return below is a refusal)
    switch (op) {
    case kOpIngest: case kOpAppend: case kOpFeed: {
        const int dtype = (int)w.size();
        const int64_t B = w.size(), n = w.size(), C = w.size();
        const int64_t st[3] = {w.size(), w.size(), w.size()};
        const Ref src = w.ref(), hi = w.ref(), lo = w.ref();
        const int es = dtype_bytes(dtype);
        if (w.bad || !es || !plane_ok(B, n, C) || B > 65535 || !A.holds(src, 0, span3(st, B, n, C), es)) return hipErrorInvalidValue;
        if (op == kOpIngest) {
            const Ref flag = w.ref(), len = w.ref();
            if (w.bad || !A.holds(hi, 0, B * n * C, 4) || (dtype == REPET_F64 && !A.holds(lo, 0, B * n * C, 4)) ||
                !A.null_or_holds(flag, 0, 1, 4) || !A.null_or_holds(len, 0, B, 8))
                return hipErrorInvalidValue;
            refused = false;
            return launch_ingest(A.at_bytes(src, es), dtype, (int32_t)B, n, (int32_t)C, st, A.at<float>(hi), A.at<float>(lo),
                                 A.at<unsigned int>(flag), A.at<int64_t>(len), s);
        }
        if (op == kOpAppend) {
            const int64_t d_stream = w.size(), d_off = w.size();
            const int64_t end = (B - 1) * d_stream + d_off + n * C;
            if (w.bad || !A.holds(hi, 0, end, 4) || !A.holds(lo, 0, end, 4)) return hipErrorInvalidValue;
            refused = false;
            return launch_stream_append(A.at_bytes(src, es), dtype, (int32_t)B, n, (int32_t)C, st, A.at<float>(hi), A.at<float>(lo), d_stream, d_off, s);
        }
        const int64_t ring_stride = w.size(), ring_len = w.size();
        if (w.bad || 3 * B > w.n - w.at) return hipErrorInvalidValue;                     // (three lists of B words follow)
        std::vector<int32_t> slots((size_t)B);
        std::vector<int64_t> counts((size_t)B), wpos((size_t)B);
        int64_t top = 0;
        for (auto& v : slots) { v = (int32_t)w.size(); top = std::max<int64_t>(top, v); }
        for (auto& v : counts) v = w.off();
        for (auto& v : wpos) v = w.off();
        if (w.bad || top > 65535 || !A.holds(hi, 0, (top + 1) * ring_stride, 4) || !A.holds(lo, 0, (top + 1) * ring_stride, 4))
            return hipErrorInvalidValue;
        refused = false;
        return launch_feed(A.at_bytes(src, es), dtype, n, (int32_t)C, st, slots.data(), counts.data(), wpos.data(), (int32_t)B, A.at<float>(hi),
                           A.at<float>(lo), ring_stride, ring_len, s);
    }
    case kOpEgress: {
        const int dtype = (int)w.size();
        const int64_t S = w.size(), n = w.size(), C = w.size();
        const int64_t st[3] = {w.size(), w.size(), w.size()};
        const Ref in = w.ref(), dst = w.ref();
        const int es = dtype_bytes(dtype);
        if (w.bad || !es || !plane_ok(S, n, C) || !A.holds(in, 0, S * n * C, 4) || !A.aligned(in, 4, 16) ||
            !A.holds(dst, 0, span3(st, S, n, C), es))
            return hipErrorInvalidValue;
        refused = false;
        return launch_stream_egress(A.at<float>(in), (int32_t)S, n, (int32_t)C, A.at_bytes(dst, es), dtype, st, s);
    }
    case kOpEmit: case kOpLevels: {
        const int dtype = op == kOpEmit ? (int)w.size() : REPET_F64;
        const int64_t S = w.size(), n = w.size(), C = w.size(), in_stream = w.size(), pos0 = w.any(), hop = w.any();
        const Ref bg = w.ref(), hi = w.ref(), lo = w.ref(), table = w.ref(), bg_fg = w.ref(), live_len = w.ref();
        EmitGain gain;
        bool with_gain = false;
        const int es = dtype_bytes(dtype);
        if (w.bad || !es || !plane_ok(S, n, C) || S > 65535 || !read_gain(w, A, S, fv, n_fv, gain, with_gain)) return hipErrorInvalidValue;
        const int64_t per = n * C;
        if (!A.holds(bg, 0, S * per, 4) || !A.null_or_holds(bg_fg, 0, S * per, 4) || !A.holds(hi, 0, (S - 1) * in_stream + per, 4) ||
            !A.null_or_holds(lo, 0, (S - 1) * in_stream + per, 4) || !A.null_or_holds(table, 0, S, 8) || !A.null_or_holds(live_len, 0, S, 8))
            return hipErrorInvalidValue;
        if (op == kOpLevels) {
            const Ref dst = w.ref(), partial = w.ref();
            if (w.bad || !A.holds(dst, 0, S * C * REPET_LEVEL_FIELDS, 8) ||
                !A.null_or_holds(partial, 0, stream_levels_partials((int32_t)S, n, (int32_t)C), 8))
                return hipErrorInvalidValue;
            refused = false;
            return launch_stream_levels(A.at<float>(bg), A.at<float>(hi), A.at<float>(lo), in_stream, A.at<int64_t>(table), pos0, hop, (int32_t)S, n,
                                        (int32_t)C, A.at<double>(dst), A.at<double>(partial), s, with_gain ? &gain : nullptr, A.at<float>(bg_fg),
                                        A.at<int64_t>(live_len));
        }
        // (emit_body reads bg and bg_fg in whole vectors of a thread's run: 16 bytes, 8 for float64)
        if (!A.aligned(bg, 4, 16) || !A.aligned(bg_fg, 4, 16)) return hipErrorInvalidValue;
        const int64_t n_dsts = w.size();
        if (w.bad || n_dsts < 1 || n_dsts > 2) return hipErrorInvalidValue;
        EmitDst d[2];
        for (int k = 0; k < n_dsts; ++k) {
            d[k].which = (int)w.size();
            for (int q = 0; q < 3; ++q) d[k].strides[q] = w.size();
            const Ref p = w.ref();
            if (w.bad || d[k].which < REPET_OUT_BACKGROUND || d[k].which > REPET_OUT_MIXTURE || !A.holds(p, 0, span3(d[k].strides, S, n, C), es))
                return hipErrorInvalidValue;
            d[k].p = A.at_bytes(p, es);
        }
        refused = false;
        return launch_stream_emit(A.at<float>(bg), A.at<float>(hi), A.at<float>(lo), in_stream, A.at<int64_t>(table), pos0, hop, (int32_t)S, n, (int32_t)C,
                                  dtype, d, (int)n_dsts, s, with_gain ? &gain : nullptr, A.at<float>(bg_fg), A.at<int64_t>(live_len));
    }
    case kOpTailClear: {
        const int64_t B = w.size(), C = w.size(), T = w.size(), FS = w.size(), W = w.size(), H = w.size(), spec = w.size(), chan = w.size(),
                      longest = w.size();
        const Ref X = w.ref(), Mk = w.ref(), len = w.ref();
        const int64_t cells = B < 1 || C < 1 ? 0 : (B - 1) * spec + (C - 1) * chan + T * FS;
        if (w.bad || B < 1 || C < 1 || H < 1 || FS < 4 || (spec & 3) || (chan & 3) || !A.holds(X, 0, cells, 8) || !A.aligned(X, 8, 16) ||
            !A.null_or_holds(Mk, 0, cells, 4) || !A.aligned(Mk, 4, 16) || !A.holds(len, 0, B, 8))
            return hipErrorInvalidValue;
        refused = false;
        return launch_tail_clear(A.at<float2>(X), A.at<float>(Mk), spec, chan, (int32_t)B, (int32_t)C, T, (int32_t)FS, (int32_t)W, (int32_t)H,
                                 A.at<int64_t>(len), longest, s);
    }
    case kOpRowCopies: case kOpSlideHeld: {
        const int64_t n_parts = w.size(), S = w.size();
        const Ref table = w.ref();
        if (w.bad || n_parts > kRowCopyParts || S < 1 || !A.null_or_holds(table, 0, S, 8)) return hipErrorInvalidValue;
        RowCopy parts[kRowCopyParts];
        HeldShift shifts[kRowCopyParts];
        for (int k = 0; k < n_parts; ++k) {
            const Ref src = w.ref(), dst = w.ref();
            RowCopy& p = parts[k];
            p.len = w.size(); p.blocks = w.size(); p.src_block = w.size(); p.dst_block = w.size(); p.src_stream = w.size(); p.dst_stream = w.size();
            p.row_len = w.size(); p.frame0 = w.any();
            shifts[k] = HeldShift{0, 0};
            if (op == kOpSlideHeld) { shifts[k].delta = w.off(); shifts[k].zero_below = w.size(); }
            // (a held stream reads from `delta` floats further on, from element zero_below of a run)
            const int64_t low = std::min<int64_t>(0, shifts[k].delta + std::min(shifts[k].zero_below, p.len));
            if (w.bad || !A.holds(dst, 0, run_span(p.len, p.blocks, p.dst_block, S, p.dst_stream), 4) ||
                !A.null_or_holds(src, low, run_span(p.len, p.blocks, p.src_block, S, p.src_stream), 4))
                return hipErrorInvalidValue;
            p.src = A.at<float>(src); p.dst = A.at<float>(dst);
        }
        refused = false;
        if (op == kOpRowCopies) return launch_row_copies(parts, (int)n_parts, (int32_t)S, s, A.at<int64_t>(table));
        return launch_slide_held(parts, shifts, (int)n_parts, (int32_t)S, s, A.at<int64_t>(table));
    }
    case kOpSlotSet: {
        const Ref table = w.ref();
        const int64_t n_table = w.size(), n = w.count();
        std::vector<int32_t> slots((size_t)n);
        std::vector<int64_t> values((size_t)n);
        for (auto& v : slots) { v = (int32_t)w.size(); if (v >= n_table) w.bad = true; }
        for (auto& v : values) v = w.any();
        if (w.bad || n_table > 65535 || !A.holds(table, 0, n_table, 8)) return hipErrorInvalidValue;
        refused = false;
        return launch_slot_set(A.at<int64_t>(table), slots.data(), values.data(), (int32_t)n, s);
    }
    case kOpTake: {
        const int64_t n_slots = w.size(), len = w.size(), ring_stride = w.size(), ring_len = w.size(), d_stream = w.size(), d_off = w.size();
        const Ref hi = w.ref(), lo = w.ref(), dhi = w.ref(), dlo = w.ref(), table = w.ref();
        if (w.bad || n_slots > w.n - w.at) return hipErrorInvalidValue;                    // (the list of n_slots words follows)
        std::vector<int64_t> rpos((size_t)n_slots);
        for (auto& v : rpos) v = w.off();
        if (w.bad || n_slots < 1 || !A.holds(hi, 0, n_slots * ring_stride, 4) || !A.holds(lo, 0, n_slots * ring_stride, 4) ||
            !A.holds(dhi, 0, n_slots * d_stream, 4) || !A.holds(dlo, 0, n_slots * d_stream, 4) || !A.holds(table, 0, n_slots, 8))
            return hipErrorInvalidValue;
        refused = false;
        return launch_take(A.at<float>(hi), A.at<float>(lo), ring_stride, ring_len, rpos.data(), (int32_t)n_slots, len, A.at<float>(dhi),
                           A.at<float>(dlo), d_stream, d_off, A.at<int64_t>(table), s);
    }
    case kOpSlotReset: {
        const Ref table = w.ref();
        const int64_t n_table = w.size(), value = w.any(), n_slots = w.size(), n_parts = w.size();
        if (w.bad || n_slots > w.n - w.at) return hipErrorInvalidValue;                    // (the list of n_slots words follows)
        std::vector<int32_t> slots((size_t)n_slots);
        int64_t top = 0;
        for (auto& v : slots) { v = (int32_t)w.size(); top = std::max<int64_t>(top, v); }
        if (w.bad || n_parts > kRowCopyParts || n_table > 65535 || top >= n_table || !A.holds(table, 0, n_table, 8)) return hipErrorInvalidValue;
        ZeroPart parts[kRowCopyParts];
        for (int k = 0; k < n_parts; ++k) {
            const Ref dst = w.ref();
            ZeroPart& p = parts[k];
            p.len = w.size(); p.blocks = w.size(); p.dst_block = w.size(); p.dst_stream = w.size();
            if (w.bad || !A.holds(dst, 0, run_span(p.len, p.blocks, p.dst_block, top + 1, p.dst_stream), 4)) return hipErrorInvalidValue;
            p.dst = A.at<float>(dst);
        }
        refused = false;
        return launch_slot_reset(A.at<int64_t>(table), value, slots.data(), (int32_t)n_slots, parts, (int)n_parts, s);
    }
    case kOpSlotExport: case kOpSlotImport: {
        const int64_t n_parts = w.size();
        const Ref table = w.ref();
        const int64_t n_slots = w.size(), slot = w.size(), value = w.any(), shift = w.any();
        if (w.bad || n_parts > kRowCopyParts || (op == kOpSlotImport && !A.holds(table, 0, n_slots, 8))) return hipErrorInvalidValue;
        SlotMove parts[kRowCopyParts];
        for (int k = 0; k < n_parts; ++k) {
            const Ref src = w.ref(), dst = w.ref();
            SlotMove& p = parts[k];
            p.src_off = w.off(); p.len = w.size(); p.blocks = w.size(); p.src_block = w.size(); p.dst_block = w.size(); p.zero_below = w.size();
            const bool reads = src.arena >= 0 && p.zero_below < p.len;
            if (w.bad || !A.holds(dst, 0, run_span(p.len, p.blocks, p.dst_block, 1, 0), 4) ||
                (reads && !A.holds(src, p.src_off + p.zero_below, p.src_off + run_span(p.len, p.blocks, p.src_block, 1, 0), 4)))
                return hipErrorInvalidValue;
            p.src = A.at<float>(src); p.dst = A.at<float>(dst);
        }
        refused = false;
        if (op == kOpSlotExport) return launch_slot_export(parts, (int)n_parts, s);
        return launch_slot_import(parts, (int)n_parts, A.at<int64_t>(table), (int32_t)n_slots, (int32_t)slot, value, shift, s);
    }
    case kOpGainFill: {
        const Ref table = w.ref();
        const int64_t n = w.size();
        if (w.bad || n_fv < 1 || !A.holds(table, 0, n, 4)) return hipErrorInvalidValue;
        refused = false;
        return launch_gain_fill(A.at<float>(table), (int32_t)n, (float)fv[0], s);
    }
    case kOpGainSet: {
        const Ref tgt = w.ref();
        const int64_t n_table = w.size(), n = w.count();
        std::vector<int32_t> slots((size_t)n);
        std::vector<float> a((size_t)n);
        for (auto& v : slots) { v = (int32_t)w.size(); if (v >= n_table) w.bad = true; }
        if (w.bad || n_fv < n || n_table > 65535 || !A.holds(tgt, 0, n_table, 4)) return hipErrorInvalidValue;
        for (int64_t k = 0; k < n; ++k) a[(size_t)k] = (float)fv[k];
        refused = false;
        return launch_gain_set(A.at<float>(tgt), slots.data(), a.data(), (int32_t)n, s);
    }
    case kOpGainCommit: {
        const Ref tgt = w.ref(), cur_old = w.ref(), cur_new = w.ref();
        const int64_t n = w.size(), slot = w.off();
        if (w.bad || !A.holds(tgt, 0, n, 4) || !A.holds(cur_old, 0, n, 4) || !A.holds(cur_new, 0, n, 4)) return hipErrorInvalidValue;
        refused = false;
        return launch_gain_commit(A.at<float>(tgt), A.at<float>(cur_old), A.at<float>(cur_new), (int32_t)n, (int32_t)slot, s);
    }
    case kOpBandExpand: {
        const Ref tab = w.ref(), job = w.ref();
        const int64_t n_table = w.size(), FS = w.size(), F = w.size(), n = w.size(), n_bands = w.size(), rows = w.size(), init = w.size();
        if (w.bad || n < 1 || n_bands < 1 || rows < 1 || !A.holds(tab, 0, n_table * kBandRows * FS, 4) ||
            !A.holds(job, 0, band_job_words((int32_t)n, (int32_t)n_bands, (int32_t)rows), 4))
            return hipErrorInvalidValue;
        const int32_t* words = A.on_host<int32_t>(job);
        for (int64_t k = 0; k < n; ++k) if (words[k] < 0 || words[k] >= n_table) return hipErrorInvalidValue;
        refused = false;
        return launch_band_expand(A.at<float>(tab), (int32_t)FS, (int32_t)F, A.at<int32_t>(job), (int32_t)n, (int32_t)n_bands, (int32_t)rows, init != 0, s);
    }
    case kOpBandCommit: {
        const Ref tab = w.ref(), table = w.ref();
        const int64_t FS = w.size(), n_slots = w.size(), slot = w.off(), mode = w.size();
        if (w.bad || slot >= n_slots || !A.holds(tab, 0, n_slots * kBandRows * FS, 4) || !A.null_or_holds(table, 0, n_slots, 8))
            return hipErrorInvalidValue;
        refused = false;
        return launch_band_commit(A.at<float>(tab), (int32_t)FS, (int32_t)n_slots, (int32_t)slot, (int)mode, A.at<int64_t>(table), s);
    }
    default: return hipErrorInvalidValue;
    }
}
}  // namespace

extern "C" {

int repet_debug_devio_stage(repet_ctx* c, int32_t op, int32_t n_arenas, const void* const* arena_in, const int64_t* arena_bytes,
                            const int32_t* arena_shift, void* const* arena_out, int32_t prefill, const int64_t* iv, int32_t n_iv,
                            const double* fv, int32_t n_fv, int64_t* report_out) {
    if (!c || !arena_in || !arena_bytes || !arena_shift || !arena_out || !iv || !report_out || (n_fv > 0 && !fv))
        return fail(REPET_ERR_BAD_ARG, "null argument");
    if (n_arenas < 1 || n_arenas > 16 || n_iv < 0 || n_fv < 0) return fail(REPET_ERR_BAD_ARG, "1 .. 16 arenas");
    for (int k = 0; k < n_arenas; ++k) {
        const int32_t sh = arena_shift[k];
        if (arena_bytes[k] < 0 || arena_bytes[k] > ((int64_t)1 << 30) || !arena_in[k] || !arena_out[k] ||
            !(sh == 0 || sh == 2 || sh == 4 || sh == 8 || sh == 12))
            return fail(REPET_ERR_BAD_ARG, "an arena: up to 2^30 bytes, its first byte 0, 2, 4, 8 or 12 bytes behind a 256-byte boundary");
    }
    DeviceGuard guard(c->device);
    const int fill = prefill & 255;
    Arenas A(n_arenas);
    for (int k = 0; k < n_arenas; ++k) {
        const size_t k_ = (size_t)k;
        const size_t total = (size_t)round_up(kArenaGuard + arena_shift[k] + arena_bytes[k] + kArenaGuard, 256);
        HIP_TRY(A.dev[k_].b.ensure(total));
        if (reinterpret_cast<uintptr_t>(A.dev[k_].b.p) & 255) return fail(REPET_ERR_HIP, "an allocation off a 256-byte boundary");
        A.first[k_] = A.dev[k_].b.as<char>() + kArenaGuard + arena_shift[k];
        A.bytes[k_] = arena_bytes[k];
        A.shift[k_] = arena_shift[k];
        A.host[k_] = static_cast<const char*>(arena_in[k]);
        HIP_TRY(hipMemsetAsync(A.dev[k_].b.p, fill, total, c->stream));
        if (arena_bytes[k] > 0) HIP_TRY(hipMemcpyAsync(A.first[k_], arena_in[k], (size_t)arena_bytes[k], hipMemcpyHostToDevice, c->stream));
    }
    Words w{iv, n_iv};
    DevioReport report;
    bool refused = false;
    devio_report = &report;
    const hipError_t e = run_devio_op(op, A, w, fv, n_fv, c->stream, refused);
    devio_report = nullptr;
    if (refused || e == hipErrorInvalidValue) {
        (void)hipStreamSynchronize(c->stream);
        return fail(REPET_ERR_BAD_ARG, refused ? "the launch would index outside an arena (or the words do not describe the op)"
                                               : "the launcher refused its arguments");
    }
    HIP_TRY(e);
    for (int k = 0; k < n_arenas; ++k)
        HIP_TRY(hipMemcpyAsync(arena_out[k], A.first[(size_t)k] - kArenaGuard, (size_t)(arena_bytes[k] + 2 * kArenaGuard), hipMemcpyDeviceToHost,
                               c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int64_t v[24] = {};
    v[0] = report.launches;
    for (int k = 0; k < 3; ++k) v[1 + k] = report.grid[k];
    for (int k = 0; k < 2; ++k) v[4 + k] = report.dense[k];
    for (int k = 0; k < kRowCopyParts; ++k) { v[6 + k] = report.src_vec[k]; v[11 + k] = report.dst_vec[k]; v[16 + k] = report.held_vec[k]; }
    std::memcpy(report_out, v, sizeof(v));
    return REPET_OK;
}

}  // extern "C"
