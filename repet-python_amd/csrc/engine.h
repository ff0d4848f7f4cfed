// Shared by the translation units of the host orchestration (engine*.hip): the context, its workspaces, the error plumbing
// and the helpers one pipeline file calls in another.
//   engine.hip         contexts, tables, Gram / STFT wrappers, the pipelines' inverse STFT (istft_args, enqueue_istft), timing, uploads
//                      and downloads, the C ABI's core entry points (the four executes are one body: execute)
//   engine_period.hip  original, extended, adaptive (the period family)
//   engine_sim.hip     sim, simonline, the peak picking's refinement plumbing
//   engine_batch.hip   repet_run_batch over several devices, the RCCL transport
//   engine_stages.hip  stage-level exports and the accessors of a run's integer intermediates
//   engine_online.hip  the streaming handle: one body per emitting call, host and device forms alike
#pragma once
#include "../../include/repet_hip.h"
#include "common.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

namespace repet_eng {
using namespace repet;

extern thread_local std::string g_last_error;
int fail(int code, const std::string& msg);



#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            return fail(e_ == hipErrorOutOfMemory ? REPET_ERR_OOM : REPET_ERR_HIP,                 \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                        \
        }                                                                                          \
    } while (0)

#define RP_TRY(expr)                                                                               \
    do {                                                                                           \
        int rc_ = (expr);                                                                          \
        if (rc_ != REPET_OK) return rc_;                                                           \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool borrowed = false;        // points into another context's buffer: never freed or grown here
    void borrow(void* ptr, size_t bytes) { p = ptr; cap = bytes; borrowed = true; }
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (borrowed) return hipErrorInvalidValue;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        const size_t want = (bytes + 255) & ~size_t(255);
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p && !borrowed) (void)hipFree(p); p = nullptr; cap = 0; borrowed = false; }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

struct Tables {
    DevBuf window, twiddle;
    DevBuf window64, twiddle64;   // the same in float64 (second level of the peak picking, peaks_exact.hip): W and W + 1 entries
    double cola = 1.0;   // sum(window[0:W:H]) for H = W/2 (repet.py:1103)
};

}  // namespace repet_eng

using repet_eng::DevBuf;
using repet_eng::Tables;
using repet::StagingRing;

struct repet_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t side_stream = nullptr;   // short independent kernels run beside the main stream
    hipStream_t copy_stream = nullptr;   // the remainder plane of a float64 upload follows the samples here (created on first use)
    std::vector<hipStream_t> ballast_streams;   // candidates that shared the main stream's hardware queue (pick_side_stream)
    hipEvent_t fork_event = nullptr, join_event = nullptr;
    // resident clip
    DevBuf staging, audio, out, out64;
    StagingRing ring;             // pinned chunks the waveforms travel through (hostio.hip)
    int64_t n_samples = 0;        // per clip
    int32_t n_clips = 1;          // equal-shape clips back to back in `audio` / `out` (repet_ctx_upload_batch)
    int64_t clip_base = 0;        // first sample of the clip the single-clip pipelines currently work on
    // A RAGGED batch (repet_ctx_upload_device_ragged): n_samples is the PITCH of the resident batch, clip b holds clip_len[b] <=
    // n_samples live samples and the planes are zero from there to the pitch. clip_len empty: every clip is n_samples long (every
    // other upload clears it). clip_len_dev: the same table on the device, int64 [n_clips], written on the context's stream by
    // the upload -- the ingest, the emission, the levels and simonline's tail clear read it. clip_n: the LENGTH of the clip
    // run_algo's loop is working on (-1: the pitch); the pipelines take cur_n() where they mean the clip, n_samples where they
    // mean the layout.
    std::vector<int64_t> clip_len; DevBuf clip_len_dev;
    int64_t clip_n = -1;
    int64_t cur_n() const { return clip_n >= 0 ? clip_n : n_samples; }
    bool ragged() const { return !clip_len.empty(); }
    const int64_t* live_len() const { return clip_len.empty() ? nullptr : static_cast<const int64_t*>(clip_len_dev.p); }
    // repet_ctx_set_window: the resident samples are [win_offset, win_offset + n_samples) of a clip of win_total samples
    // (multi-GPU `extended`: a rank holds only the samples of its own segment range); 0 = the resident clip is whole
    int64_t win_total = 0, win_offset = 0;
    bool win_skip_clear = false;  // exec_extended cleared `out` itself (window mode)
    DevBuf Mk;                    // the soft mask as a plane of its own (laid out like V), when the inverse STFT applies it
    DevBuf Wm;                    // original / extended: the repeating-segment models [clip][channel][q][FS] when the inverse STFT applies THEM
    bool mask_model = false;      // this pipeline's inverse STFT computes the mask from V and Wm (run_original)
    bool band_lookback = false;   // the last run_gram_band wrote band[j][l] = sim(j, j - l) (simonline on the f16-split kernel)
    bool mask_plane = false;      // the pipeline being enqueued keeps the mask apart instead of multiplying X in place
    bool ola_first_batch = false; // run_original: the first batch of equal segments of an `extended` run (class 0 may store)
    int32_t last_fs = 0;          // sampling frequency of the resident clip when it came from a WAVE file (for repet_ctx_result_wav)
    // `extended`: the longer last segment cannot join the batch of equal segments; its analysis (STFT .. mask) runs on
    // this auxiliary context's stream beside the batch and only its inverse STFT waits for the batch's
    repet_ctx* aux = nullptr;
    hipEvent_t aux_start = nullptr, aux_main_done = nullptr, aux_done = nullptr;
    std::function<int()> pre_synthesis;      // run_original calls it (once) right before its inverse STFT
    bool clip_loop = false;       // true while run_algo works through the clips one by one
    int32_t last_clip_passes = 0; // how often the last execute enqueued its variant's pipeline (repet_ctx_last_clip_passes)
    // What the pass a pipeline has just enqueued left in the spectra workspaces (record_spectrum, where each exec_* ends: the
    // scopes forget the form when the pipeline returns): form 0 X masked in place, 1 X and the plane Mk, 2 X, the model Wm
    // and the period slots; nb clips of T frames each, chan_stride floats between channel planes; warm: the frames before it
    // carry no background (simonline). form -1: no pass yet.
    struct SpectrumRecord {
        int form = -1; const float* model = nullptr; const int32_t* periods = nullptr;
        int64_t model_batch_stride = 0, model_chan_stride = 0; int32_t cutoff = 0, model_rows = 0;
        int32_t W = 0, H = 0, F = 0, FS = 0, C = 0, nb = 0, centred = 1; int64_t T = 0, chan_stride = 0, warm = 0;
    } spectrum;
    // repet_ctx_request_frames: armed for exactly the next execute, which checks it against its own geometry before it enqueues
    // anything, serves it behind every pass (run_algo) and drops it, whatever becomes of the run. n_bands 0: whole frames
    // (fp32, element strides); otherwise band energies (float64, dense). n_frames: the pitch's frame count, set by the execute.
    struct FramesRequest {
        bool armed = false; int which = 0; int32_t n_bands = 0; int32_t edges[REPET_MAX_BANDS + 1] = {};
        void* dst = nullptr; int64_t strides[4] = {0, 0, 0, 0}; void* signal_stream = nullptr; int64_t n_frames = 0;
    } frames_req;
    int32_t n_channels = 0;
    bool strict = true;           // samples that are not finite are let through as repet.py lets them (all five variants); false: REPET_FLAG_REFUSE_NONFINITE
    bool input_not_finite = false;   // the resident clip came from a host array that held such samples
    // the resident clip was never scanned (device planes -- the RCCL transport, torch tensors --, float WAVE payloads): under
    // `strict` the passes that reproduce the reference on such samples then run unconditionally (they cost microseconds)
    bool input_unscanned = false;
    // device-side ingest / egress of caller buffers (devio.hip): the context's stream waits on io_wait recorded on the
    // caller's stream, the caller's stream on io_done recorded behind the egress; the refusal mode's non-finite flag word
    hipEvent_t io_wait = nullptr, io_done = nullptr;
    DevBuf nonfinite_word;
    DevBuf levels_ws;             // level records on their way to the host and the chunk partials of the level reduction (devio.hip)
    int result_which = REPET_OUT_BACKGROUND;   // what repet_ctx_download_device_strided writes (repet_ctx_select_result)
    // repet_ctx_set_background_gain: the foreground it writes is x - result_a * bg, result_a = (float)(1 - gain); off: x - bg as ever
    float result_a = 1.f; bool result_gain = false;
    // repet_ctx_set_background_band_gains: a table g[row][k < F] (host copy band_g; band_rows 0: never set or cleared) and
    // its factors a = (float)(1 - (double)g) on the device, band_tab[row][FS] (written on the context's stream where the
    // table is set, so behind every run enqueued before). A run enqueued while a table with a gain other than 0 is set
    // (band_any) is `run_shaped`: behind every inverse STFT of the pipeline a second one, with the factor rows beside whatever
    // mask form the first took, writes the SHAPED background into out_fg. result_shaped: out_fg belongs to the resident
    // result -- the foreground and its levels are formed from it (bg_fg of the emission kernels) until the next execute or upload.
    std::vector<float> band_g; int32_t band_W = 0, band_rows = 0; bool band_any = false;
    DevBuf band_tab, out_fg;
    bool run_shaped = false, result_shaped = false;
    const float* shaped_bg() const { return result_shaped ? static_cast<const float*>(out_fg.p) : nullptr; }
    int online_start = 0;        // simonline: start_frames of this context (repet_ctx_set_online_start; 0: buffer_frames, the reference)
    // REPET_FLAG_SILENT_FRAMES_ZERO, for the simonline pipeline or live push being enqueued (SilentZeroScope): run_stft has the
    // forward kernel flag the silent frames in `silent` (one word per frame row of the launch), make_refine and run_exact_rows
    // hand the rule to the peak picking, and the pipeline gives the table to the mask kernels
    bool silent_zero = false;
    DevBuf silent;
    bool nonfinite_passes() const { return input_not_finite || (strict && input_unscanned); }
    // workspaces
    DevBuf X, V, Vn, P, S, band, beat, idx, cnt, periods, win_periods, frames, tmp_a, tmp_b, tmp_c;
    DevBuf peak_scratch;          // per-segment candidates of long similarity rows (launch_local_maxima)
    DevBuf seg;                   // segment records of the similarity rows (PeakArgs::seg): [row][m1 | m2 | arg][seg_pitch]
    DevBuf beat_partial;          // chunk sums of the beat-spectrum windows (launch_band_window_sum)
    DevBuf amax;                  // inverse scale of every row of the matrix being split (scaled f16-split band Gram)
    DevBuf Vh;                    // f16 hi / lo halves of Vn for the split-precision Gram (gram_f16.hip)
    DevBuf refine_stats;          // kRefineStats counters of the last sim/simonline run (PeakRefine::stats)
    // second level of the peak picking (peaks_exact.hip): the fp32 remainders of a float64 upload (audio = hi, audio_lo = lo,
    // hi + lo = 48 bits of the caller's sample; empty when every remainder was zero or the input was not float64), the rows
    // handed over, the table of float64 unit rows with its generation stamps, the row workspaces of the fixed grid
    DevBuf audio_lo; bool has_lo = false;
    DevBuf redo_list, redo_flag, u64, u64_gen, exact_scratch;
    DevBuf lite_list, lite_flag, lite_records, frame_list, frame_flag;   // the wavefront kernel's fast path (peaks_wave.hip)
    unsigned int exact_gen = 0;
    bool refine_stats_cleared = false;   // ensure_spectra's housekeeping launch has zeroed them for the run being enqueued
    DevBuf R, Vs, rank_codes;     // rank codes of V, the sorted columns and the column-major codes (rank-domain median of `sim`, rank.hip)
    DevBuf code_planes, median_codes;   // the same codes bit-sliced, and the selected codes per cell (mask_bits.hip)
    // geometry for which the constant median-pad rows of R are in place (they survive every run of that geometry)
    const void* r_pads_ptr = nullptr; int64_t r_pads_stride = 0, r_pads_row = 0; int r_pads_channels = 0, r_pads_fs = 0;
    std::map<int, std::unique_ptr<Tables>> tables;
    // Gram tile lists by (nb, ndiag), kept side by side: variants that alternate on one context (each with its own list) do
    // not rebuild one -- and wait for the stream to drain before overwriting it -- on every call
    struct TileList { DevBuf buf; int count = 0; };
    std::map<std::pair<int, int>, TileList> tile_lists;
    DevBuf tiles_big;             // upper-triangle list of 256 x 256 tiles (gram_f16_big.hip)
    int tiles_big_nb = -1, tiles_big_count = 0;
    // last run
    int last_algo = -1;
    int64_t last_T = 0;
    int32_t last_n_periods = 0;
    int64_t last_idx_rows = 0;
    int32_t last_idx_pitch = 0;
    int32_t last_idx_number = 0;
    int32_t last_FS = 0; int64_t last_chan_stride = 0;     // sim: geometry of the last run's per-cell arrays
    int32_t last_median_path = 0;     // sim: 0 selection on the float magnitudes, 1 packed network on rank codes, 2 bit-sliced selection
    int32_t last_idx_batch = 1;   // clips whose lists sit back to back in idx / cnt (batch contexts)
    bool band_on_f16 = false;     // the last banded Gram ran on the f16-split kernel (stage label / roofline of bench.py)
    // timing
    std::vector<hipEvent_t> events;
    repet_timing* timing = nullptr;
    int n_marks = 0;
    // timing series (repet_ctx_timing_series_begin): every asynchronous run records its own block of events
    bool series_on = false; int series_cap = 0, series_steps = 0, series_marks = 0, event_base = 0;
    repet_timing series_timing{};
};

namespace repet_eng {

struct DeviceGuard {
    int prev = 0;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && hipSetDevice(dev) == hipSuccess) ok = true;
    }
    ~DeviceGuard() { if (ok) (void)hipSetDevice(prev); }
};

struct Geo {
    int W, H, F, FS;
    int64_t T, Tpad, chan_stride;
    int C;
};

enum class MaskKind { period, adaptive, sim_float, sim_ranks };

struct MaskPlaneScope {            // the choice holds for one pipeline; stage exports and the streaming handle never see it
    repet_ctx* c;
    MaskPlaneScope(repet_ctx* ctx, bool on) : c(ctx) { c->mask_plane = on; }
    ~MaskPlaneScope() { c->mask_plane = false; }
};

struct SilentZeroScope {           // the rule holds for one pipeline, like the mask plane
    repet_ctx* c;
    SilentZeroScope(repet_ctx* ctx, bool on) : c(ctx) { c->silent_zero = on; }
    ~SilentZeroScope() { c->silent_zero = false; }
};

struct ModelRef { const float* model; const int32_t* periods; int64_t batch_stride, chan_stride; int32_t cutoff; };

struct BatchInfo { int64_t transport = 0, clips_sent = 0, clips_with_remainders = 0, groups = 0; };
extern thread_local BatchInfo g_batch_info;

int logical_device_count(int physical);
int run_batch_impl(int algo, int32_t n_clips, const void* const* audio, int dtype, const int64_t* n_samples,
                   const int32_t* n_channels, const repet_params* p, double* const* out, int32_t n_devices, int transport,
                   int one_device = -1);
void release_stream_contexts();
float peak_refine_delta(int FS, bool f16_gram);
double peak_exact_delta2();
int ensure_stamps(repet_ctx* c, DevBuf& buf, size_t count);
int make_refine(repet_ctx* c, const float* unit_rows, int FS, double threshold, PeakRefine* rf, int64_t rows = 0, int clips = 1,
                int n_cols = 0, int d = 0, int64_t frames = 0);
int run_exact_rows(repet_ctx* c, const Tables* tb, const Geo& g, const float* M, int64_t row0, int n_cols, int64_t pitch, int mode,
                   float min_value, int d, int number, int32_t* idx, int idx_pitch, int32_t* count, int64_t shift,
                   const PeakRefine& rf, const PeakBatch* batch, const float* hi, const float* lo, int64_t n_samples,
                   int64_t clip_stride, int64_t frame_sample0, int64_t n_frames, int clips, PeakLaunch* info = nullptr);
bool rank_median_enabled();
int run_rank_columns(repet_ctx* c, const Geo& g, MaskArgs* m, hipStream_t stream, bool with_mark, int max_count);
int exec_sim(repet_ctx* c, const repet_params* p);
int exec_simonline(repet_ctx* c, const repet_params* p);
int prepare_power_planes(repet_ctx* c, const Geo& g, int64_t T, int B);
IstftOlaArgs reg_probe(int W, int channels, bool weighted, int64_t n_out, int64_t out_stride, int64_t overlap);
int run_original(repet_ctx* c, const repet_params* p, int64_t offset, int64_t n, int B, int64_t hop,
                 int32_t* period_slots, bool weighted, int seg_first, int seg_total, int64_t overlap);
int exec_original(repet_ctx* c, const repet_params* p);
int64_t extended_segment_count(int64_t N, const repet_params* p);
int exec_extended(repet_ctx* c, const repet_params* p, int64_t first = 0, int64_t n_seg = -1);
int exec_extended_plan(repet_ctx* c, const repet_params* p, int64_t first, int64_t n_seg, int64_t N);
int exec_adaptive(repet_ctx* c, const repet_params* p);
int check_params(const repet_params* p);
int check_algo_flags(int algo, const repet_params* p);
int check_clip_lengths(int algo, const repet_params* p, int32_t start_frames, const int64_t* lengths, int32_t n_clips);
int h2d_pitched(repet_ctx* c, float* dst, int64_t dpitch, const float* src, int64_t rows, int64_t cols, int64_t rows_pad);
int d2h_pitched(repet_ctx* c, float* dst, const float* src, int64_t spitch, int64_t rows, int64_t cols);
int ctx_create(int device, repet_ctx** out, bool probe_side_stream);
int run_algo_one(repet_ctx* c, int algo, const repet_params* p);
// the tensor calls' requests (engine.hip, beside run_algo): what a pass left (every exec_* records it where it ends), the frame
// grid of a variant, and the launch behind a pass whose first clip is clip `clip0` of the destination
void record_spectrum(repet_ctx* c, const Geo& g, int nb, int64_t warm, int centred, const ModelRef* mr, int model_rows);
int64_t result_frame_count(int algo, const repet_params* p, int64_t n_samples);
int serve_requests(repet_ctx* c, int clip0);
int run_algo(repet_ctx* c, int algo, const repet_params* p);
int get_tables(repet_ctx* c, int W, Tables** out);
int upload_twiddle_only(repet_ctx* c, int W, const float2** tw);
int get_tiles(repet_ctx* c, int64_t T, int ndiag, const int2** tiles, int* count);
int run_band_window_sum(repet_ctx* c, const float* band, int64_t T, int LP, int n_lags, int n_freq, int64_t start0,
                        int64_t step, int64_t len, int n_windows, float* beat, int beat_pitch, int n_batch,
                        int64_t band_batch_stride, int64_t beat_batch_stride);
bool gram_f16_enabled();
bool gram_big_enabled();
// run_gram_full = the choice of a form (gram_full_form) + its execution (exec_gram_full)
enum GramFullForm { kFullAuto = 0, kFullF32 = 1, kFullF16 = 2, kFullF16Big = 3 };
bool gram_segments_in_epilogue();
int gram_full_form(int64_t T, bool unit_rows);
int exec_gram_full(repet_ctx* c, int form, const float* A, int64_t T, int FS, float* S, int64_t TS, bool planes_ready, float* seg,
                   int seg_pitch, bool* seg_written, bool seg_in_epilogue);
int run_gram_full(repet_ctx* c, const float* A, int64_t T, int FS, float* S, int64_t TS, bool unit_rows = false,
                  bool planes_ready = false, float* seg = nullptr, int seg_pitch = 0, bool* seg_written = nullptr);
bool band_rows_on_f16(repet_ctx* c, int64_t T, int FS, int n_lags, int B, int64_t a_stride);
// run_gram_band = the choice of a form (gram_band_form) + its execution (exec_gram_band)
enum GramBandForm { kBandAuto = 0, kBandF32 = 1, kBandF16Rows = 2, kBandF16Unit = 3, kBandF16UnitLookback = 4 };
int gram_band_form(repet_ctx* c, int64_t T, int FS, int n_lags, bool unit_rows, int B, int64_t a_stride, bool planes_ready, bool lookback);
int exec_gram_band(repet_ctx* c, int form, const float* A, int64_t T, int FS, float* band, int n_lags, int LP, int B, int64_t a_stride,
                   int64_t band_stride, bool planes_ready);
int run_gram_band(repet_ctx* c, const float* A, int64_t T, int FS, float* band, int n_lags, int LP, bool unit_rows = false,
                  int B = 1, int64_t a_stride = 0, int64_t band_stride = 0, bool planes_ready = false, bool lookback = false);
void mark(repet_ctx* c, const char* name, double bytes, double flops);
void begin_timing(repet_ctx* c, repet_timing* t);
void end_timing(repet_ctx* c);
Geo make_geo(int W, int H, int64_t T, int C);
bool split_in_stft(int B);
int mask_plane_forced();
bool mask_plane_wanted(MaskKind kind);
int ensure_spectra(repet_ctx* c, const Geo& g, bool want_vn, bool want_p, int B = 1, bool p_planes = false);
int run_stft(repet_ctx* c, const Geo& g, const Tables* tb, int64_t offset, int64_t n, int centred, bool vn, bool p,
             int B = 1, int64_t batch_sample_stride = 0, bool p_as_planes = false);
MaskArgs mask_args(repet_ctx* c, const Geo& g, int cutoff);
// The inverse STFT of a pipeline (engine.hip, beside mask_args). istft_args: what every pipeline derives from the context --
// spectra, the mask plane or null, strides, channels, T / FS / W, twiddles, out = c->out, scale; the caller adds what is its own
// (trim, n_out, out_offset, accumulate_weighted, fades, the residue-class fields of `extended`). istft_clips: the batch fields of
// `count` independent clips, no cross-fade. istft_rc: the launcher's hipError_t as a return code (its refusal is REPET_ERR_LIMIT).
// enqueue_istft: the `n_launches` prepared launches of one pipeline, the timing marks scaled by `count` clips or segments of
// n_out samples and, under band gains, the shaped twins. run_istft: one clip through all of it.
IstftOlaArgs istft_args(repet_ctx* c, const Geo& g, const Tables* tb);
void istft_clips(IstftOlaArgs& a, int count, int64_t spec_stride, int64_t out_stride);
int istft_rc(hipError_t e);
void apply_model(IstftOlaArgs& a, repet_ctx*, const ModelRef* mr);
int enqueue_istft(repet_ctx* c, const Geo& g, const IstftOlaArgs* launches, int n_launches, int count, int64_t n_out);
int run_istft(repet_ctx* c, const Geo& g, const Tables* tb, int64_t trim, int64_t n_out, int64_t out_offset,
              bool weighted, int64_t fade_in, int64_t fade_out, const ModelRef* mr = nullptr);
// the shaped background of a run under band gains (engine.hip, beside run_istft): the checks and the buffer before anything is
// enqueued, the twin of a clear of `out` (values, not samples); the twins of the inverse STFTs are enqueue_istft's
int begin_shaped(repet_ctx* c, const repet_params* p);
int clear_shaped(repet_ctx* c, int64_t first_value, int64_t n_values);
// device-side I/O (devio.hip): argument checks of caller layouts, the context's ordering events and the two waits made of them
int check_strides(const int64_t* strides);
int check_no_overlap(const int64_t* strides, int32_t n_clips, int64_t n, int32_t ch);
int ensure_io_events(repet_ctx* c);
// the context's stream behind what the caller's stream(s) have enqueued so far (the producer of a source, earlier users of a
// destination; the same stream twice is recorded and waited for once), and the caller's stream behind what the context's has
int wait_caller(repet_ctx* c, void* wait_stream, void* signal_stream);
int signal_caller(repet_ctx* c, void* signal_stream);
// a background gain g in [0, 1] (BAD_ARG otherwise, NaN included) and what the egress multiplies the background by: (float)(1 - g)
int check_background_gain(float gain);
float background_gain_factor(float gain);
// What the launchers of devio.hip (below) decided, for the stage entry of this family (repet_debug_devio_stage, engine_stages.hip): while
// devio_report points at a record, every launch of devio.hip notes its grid there and counts, and the launchers note their own
// dense / src_vec / dst_vec / held_vec decisions as they pass them to the kernels (-1: not decided by this call). Null otherwise.
struct DevioReport {
    int64_t launches = 0;
    int64_t grid[3] = {0, 0, 0};                                  // of the last launch
    int64_t dense[2] = {-1, -1};
    int64_t src_vec[5] = {-1, -1, -1, -1, -1}, dst_vec[5] = {-1, -1, -1, -1, -1}, held_vec[5] = {-1, -1, -1, -1, -1};
};
extern thread_local DevioReport* devio_report;
// the streaming handle's per-push data movement (devio.hip), n_streams streams at per-stream element strides:
//   append   chunk [S][n][C] (strided, any device dtype) -> hi / lo at s * dst_stream + dst_off (fp32 + fp32 remainder)
//   copies   up to kRowCopyParts parts of `blocks` runs of `len` floats per stream (src null: zeros), one launch
//   egress   fp32 [S][n][C] -> strided F64 / F32 / I16 / F16 / BF16 destination
//            a part with row_len > 0 covers frame rows of row_len floats, the first of them frame `frame0`: of stream b only
//            the rows of frames before slot_start[b] are written (the rows of a slot whose own stream has not begun)
//   reset    the named slots' own stream begins at frame `value` (kSlotIdle: never): slot_start[slot] = value and up to
//            kRowCopyParts runs of zeros per slot (ZeroPart, strides as RowCopy's), one launch per kSlotResetIds slots
struct RowCopy { const float* src; float* dst; int64_t len, blocks, src_block, dst_block, src_stream, dst_stream; int64_t row_len = 0, frame0 = 0; };
constexpr int kRowCopyParts = 5;
static_assert(sizeof(DevioReport::src_vec) / sizeof(int64_t) == kRowCopyParts, "DevioReport holds one entry per part");
struct ZeroPart { float* dst; int64_t len, blocks, dst_block, dst_stream; };
constexpr int kSlotResetIds = 256;
constexpr int64_t kSlotIdle = (int64_t)1 << 60;
hipError_t launch_slot_reset(int64_t* slot_start, int64_t value, const int32_t* slots, int32_t n_slots, const ZeroPart* parts,
                             int n_parts, hipStream_t s);
//   hold     a HELD slot (repet_online_hold_streams) reads kSlotHeld in the table: past kSlotIdle, so every kernel that is given
//            the table treats it as idle, and the slide can tell the two apart. set: slot_start[slots[k]] = values[k] (kSlotHeld,
//            or the slot's own first frame at the resume), one launch per kSlotResetIds slots. slide: launch_row_copies with
//            copying parts only, where a held stream's element i of a run comes from shifts[part].delta (<= 0) floats further
//            on in the source for i >= zero_below and is zero below it (the source is not read there); one launch
constexpr int64_t kSlotHeld = kSlotIdle + 1;
struct HeldShift { int64_t delta, zero_below; };
hipError_t launch_slot_set(int64_t* slot_start, const int32_t* slots, const int64_t* values, int32_t n_slots, hipStream_t s);
hipError_t launch_slide_held(const RowCopy* parts, const HeldShift* shifts, int n_parts, int32_t n_streams, hipStream_t s,
                             const int64_t* slot_start);
//   feed     the per-slot inboxes (repet_online_enable_feed): slot b's ring of ring_len floats per plane at b * ring_stride of hi /
//            lo. feed: row r of the source [n_rows][n][C] (strided, any ingest dtype) brings its first counts[r] samples to the
//            ring of slots[r] from float wpos[r] on, converted as append converts. take: `len` floats of both planes from float
//            rpos[b] of every slot's ring to dst_hi / dst_lo at b * dst_stream + dst_off, except for the slots that read idle
//            or held in the table. Positions travel in the kernel arguments; both wrap; one launch per kSlotResetIds slots
hipError_t launch_feed(const void* src, int dtype, int64_t n, int32_t ch, const int64_t src_strides[3], const int32_t* slots,
                       const int64_t* counts, const int64_t* wpos, int32_t n_rows, float* hi, float* lo, int64_t ring_stride,
                       int64_t ring_len, hipStream_t s);
hipError_t launch_take(const float* hi, const float* lo, int64_t ring_stride, int64_t ring_len, const int64_t* rpos, int32_t n_slots,
                       int64_t len, float* dst_hi, float* dst_lo, int64_t dst_stream, int64_t dst_off, const int64_t* slot_start,
                       hipStream_t s);
//   export   ONE slot's share of the handle's buffers gathered into a dense payload, one launch: up to kRowCopyParts parts of
//            `blocks` runs of `len` floats; element i of a run is src[src_off + blk * src_block + i] for i >= zero_below and
//            zero below it (a run right-aligned on what the source holds: src_off may be negative, src null with zero_below = len)
//   import   the same parts the other way (payload -> slot), slot_start[slot] = value and, where the handle's epoch moves
//            with the import, slot_start[s] += shift for every other live slot: one launch
struct SlotMove { const float* src; int64_t src_off; float* dst; int64_t len, blocks, src_block, dst_block, zero_below; };
hipError_t launch_slot_export(const SlotMove* parts, int n_parts, hipStream_t s);
hipError_t launch_slot_import(const SlotMove* parts, int n_parts, int64_t* slot_start, int32_t n_slots, int32_t slot, int64_t value,
                              int64_t shift, hipStream_t s);
hipError_t launch_stream_append(const void* src, int dtype, int32_t n_streams, int64_t n, int32_t ch, const int64_t src_strides[3],
                                float* hi, float* lo, int64_t dst_stream, int64_t dst_off, hipStream_t s);
hipError_t launch_row_copies(const RowCopy* parts, int n_parts, int32_t n_streams, hipStream_t s, const int64_t* slot_start = nullptr);
//   ingest   source [n_clips][n][ch] (strided, any ingest dtype) -> hi fp32 interleaved and, for float64, the remainders lo;
//            flag (nullable): set to 1 where a live float sample is not finite; len_dev (nullable): the ragged form, clip b live
//            below sample len_dev[b]. hi / lo 16-byte aligned. One launch
hipError_t launch_ingest(const void* src, int dtype, int32_t n_clips, int64_t n, int32_t ch, const int64_t strides[3], float* hi,
                         float* lo, unsigned int* flag, const int64_t* len_dev, hipStream_t s);
hipError_t launch_stream_egress(const float* in, int32_t n_streams, int64_t n, int32_t ch, void* dst, int dtype,
                                const int64_t strides[3], hipStream_t s);
//   emit     background / foreground / mixture of an emission (or of an offline result) into one or two strided destinations
//            of one dtype, one launch: bg fp32 [S][n][C]; the input hi (+ lo, nullable) with stream s at s * in_stream floats
//            gain (nullable: the foreground is x - bg as ever): the foreground is x - a * bg, with a the scalar (offline) or
//            per stream from fp32 tables [n_streams]: a_tgt[s] from sample `ramp` - 1 of the emission on, a linear fade from
//            a_cur[s] before it (ramp 0: a_tgt everywhere)
//            bg_fg (nullable, laid out like bg): the background the FOREGROUND is formed from where it is not bg itself -- the
//            shaped one of a live handle with band gains; the background and the mixture never read it
struct EmitDst { void* p = nullptr; int which = -1; int64_t strides[3] = {0, 0, 0}; };
struct EmitGain { const float* a_cur = nullptr; const float* a_tgt = nullptr; int64_t ramp = 0; float a = 1.f; bool scalar = false; };
hipError_t launch_stream_emit(const float* bg, const float* hi, const float* lo, int64_t in_stream, const int64_t* slot_start,
                              int64_t pos0, int64_t hop, int32_t n_streams, int64_t n, int32_t ch, int dtype, const EmitDst* dsts,
                              int n_dsts, hipStream_t s, const EmitGain* gain = nullptr, const float* bg_fg = nullptr,
                              const int64_t* live_len = nullptr);
//   levels   the REPET_LEVEL_FIELDS float64 values per stream and channel of the emission the same arguments describe to
//            launch_stream_emit (include/repet_hip.h: energies, peaks, live and non-finite samples), dense [n_streams][ch][8]
//            into dst: one launch over (chunk of kLevelChunk samples, stream), and for more than one chunk a second small one
//            that folds partials [n_streams][ch][chunks][8] (stream_levels_partials doubles; 0: not needed) in a fixed order.
//            No element at all: dst is zeroed by a memset. hipErrorNotSupported: more channels than a tile holds (1024)
constexpr int64_t kLevelChunk = REPET_LEVEL_CHUNK;
int64_t stream_levels_partials(int32_t n_streams, int64_t n, int32_t ch);
hipError_t launch_stream_levels(const float* bg, const float* hi, const float* lo, int64_t in_stream, const int64_t* slot_start,
                                int64_t pos0, int64_t hop, int32_t n_streams, int64_t n, int32_t ch, double* dst, double* partials,
                                hipStream_t s, const EmitGain* gain = nullptr, const float* bg_fg = nullptr,
                                const int64_t* live_len = nullptr);
//   tail     simonline over a ragged batch: rows [T_b, T) of every clip's and channel's spectra X (and of the mask plane Mk,
//            nullable) are stored zero, T_b = repet_frame_count(lengths_dev[b], W, H, 0) read on the device; longest_tail: the
//            largest T - T_b of the batch (the host knows the lengths), which sizes the grid. One launch, none for 0
hipError_t launch_tail_clear(float2* X, float* Mk, int64_t spec_stride, int64_t chan_stride, int32_t n_clips, int32_t ch, int64_t T,
                             int32_t FS, int32_t W, int32_t H, const int64_t* lengths_dev, int64_t longest_tail, hipStream_t s);
//   gains    the background gains of the streaming handle, fp32 [S] tables of a = (float)(1 - gain). fill: n entries = a.
//            set: tgt[slots[k]] = a[k], one launch per kSlotResetIds slots named. commit: cur_new[s] = tgt[s] for the slots an
//            emission covers (slot < 0: all), cur_old[s] for the others; one launch
hipError_t launch_gain_fill(float* table, int32_t n, float a, hipStream_t s);
hipError_t launch_gain_set(float* tgt, const int32_t* slots, const float* a, int32_t n_slots, hipStream_t s);
hipError_t launch_gain_commit(const float* tgt, const float* cur_old, float* cur_new, int32_t n_slots, int32_t slot, hipStream_t s);
//   bands    the band gains of the streaming handle (repet_online_set_background_band_gains): per slot three rows of FS fp32
//            factors a[k] = (float)(1 - (double)g[k]), tab[slot][kBandCarried | kBandNew | kBandPending][FS] -- the table of the
//            frame carried over from the last push, of the frames a push completes, and of the last set.
//            expand: the pending row of the n named slots from band gains. `job` is memory the DEVICE reads (the caller's to
//            keep until the launch has run), int32 / fp32 words: slot[n] | row[n] (the row of `gains` the slot takes; < 0: every
//            g = 0) | edges[n_bands + 1] | gains[rows][n_bands]; bin k takes the gain of the band [edges[b], edges[b + 1]) that
//            holds it, 0 outside all of them and for the pad bins. init: the other two rows of the named slots are written 1
//            (a handle's first set names every slot: the tables begin there). One launch.
//            commit, for every slot (slot < 0) that is not held in slot_start (nullable) or for the one slot named, one launch:
//            kBandCommit carried = new, new = pending (a call that completes frames); kBandCarry carried = new (one that only
//            inverts the carried frame); kBandSettle carried = new = pending (a stream that moves into the slot).
constexpr int kBandCarried = 0, kBandNew = 1, kBandPending = 2, kBandRows = 3;
constexpr int kBandCommit = 0, kBandSettle = 1, kBandCarry = 2;
int64_t band_job_words(int32_t n, int32_t n_bands, int32_t rows);
hipError_t launch_band_expand(float* tab, int32_t FS, int32_t F, const int32_t* job, int32_t n, int32_t n_bands, int32_t rows, bool init,
                              hipStream_t s);
hipError_t launch_band_commit(float* tab, int32_t FS, int32_t n_slots, int32_t slot, int mode, const int64_t* slot_start, hipStream_t s);
//   frames   (frames.hip) the spectra of the frames a push completed, read from the window it wrote: V / X at the first of the
//            n_frames rows of slot 0's plane 0 (`plane` / `spec` elements between channel planes / slots), handle frame frame0
//            in that row, `warm` = start_frames - 1, slot_start nullable (every slot's stream is the handle's). frames: fp32
//            `which` of every (slot, frame, channel, bin < F) into dst at element strides [4]; bands: the float64 sums of
//            their squares over bins [edges[k], edges[k + 1]), dense [n_streams][n_frames][C][n_bands], the edges in the
//            kernel arguments. One launch each, none for n_frames == 0; hipErrorInvalidValue for edges out of order or range
struct FrameArgs {
    const float* V; const float2* X; int64_t plane, spec; int32_t FS, F, C, which; int64_t n_frames, frame0, warm;
    const int64_t* slot_start;
};
hipError_t launch_online_frames(const FrameArgs& a, int32_t n_streams, float* dst, const int64_t strides[4], hipStream_t s);
hipError_t launch_online_bands(const FrameArgs& a, int32_t n_streams, const int32_t* edges, int32_t n_bands, double* dst, hipStream_t s);
//   result   (result_frames.hip) the spectra of the pass an offline pipeline has just enqueued, in the form it left them (0 in
//            place, 1 with the plane Mk, 2 with the model rows and the clips' periods): n_frames rows are written per clip, the
//            rows below `live` -- the pass's own frame count, further lowered per clip by lengths_dev (nullable: the sample counts
//            of a ragged batch, turned into frame counts with W, H, centred) -- from the workspaces, the others zero; rows below
//            `warm` have no background. frames: fp32 at element strides [4] (clip, frame, channel, bin); bands: float64, dense
//            [n_frames][C][n_bands] per clip, clips clip_stride doubles apart. One launch each, none for n_frames == 0
struct ResultFrameArgs {
    const float* V; const float2* X; const float* Mk; const float* model; const int32_t* periods;
    int64_t chan_stride, spec_stride, model_batch_stride, model_chan_stride;
    int32_t FS, F, C, which, form, cutoff, model_rows;
    int64_t n_frames, live, warm;
    const int64_t* lengths_dev; int32_t W, H, centred;
};
hipError_t launch_result_frames(const ResultFrameArgs& a, int32_t n_clips, float* dst, const int64_t strides[4], hipStream_t s);
hipError_t launch_result_bands(const ResultFrameArgs& a, int32_t n_clips, const int32_t* edges, int32_t n_bands, double* dst,
                               int64_t clip_stride, hipStream_t s);
//   matches  (matches.hip) the similar-frame lists of the frames a push completed, read from what its peak picking left: list
//            row r of slot s at idx + s * idx_stride + r * idx_pitch (cnt likewise), for record frame n_frames - n_active + r;
//            the entries are window rows, record frame 0 being row `hist`; band: the similarities, LP lags per row, in the
//            look-back layout (band[j][l] = sim(j, j - l)) or the diagonal one (band[t][l] = sim(t, t + l)). Per (slot, frame):
//            count, and K ages (ascending, -1 behind the list) and similarities (0 behind it), dense [n_streams][n_frames](K).
//            A row of an idle or held slot, before the slot's own frame `warm`, or of a push that picked no peaks (n_active
//            == 0: idx, cnt and band are not read) is empty. One launch, none for n_frames == 0
struct MatchArgs {
    const int32_t* idx; const int32_t* cnt; const float* band; int64_t idx_stride, cnt_stride, band_stride;
    int32_t idx_pitch, LP, K, lookback; int64_t n_frames, n_active, hist, frame0, warm;
    const int64_t* slot_start;
};
hipError_t launch_online_matches(const MatchArgs& a, int32_t n_streams, int32_t* count, int32_t* age, float* similarity, hipStream_t s);
// bytes of an element of a REPET_* dtype (0: not a dtype), and the refusal of a destination dtype the emission does not write
int dtype_bytes(int dtype);
int check_emit_dtype(int dtype);
int check_disjoint(const void* p0, const int64_t* st0, const void* p1, const int64_t* st1, int elem_bytes, int32_t n_clips, int64_t n,
                   int32_t ch);
constexpr int kRankMinList = 24;     // shortest list bound for which the column sort is worth its time

}  // namespace repet_eng
