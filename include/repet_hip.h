/*
 * repet_hip.h -- C ABI of librepet_hip.so, the MI355X (gfx950) REPET separation engine.
 *
 * The reference (zafarrafii/REPET-Python, repet.py) has no FFI seam: its boundary is the Python call
 *   repet.<original|extended|adaptive|sim|simonline>(audio_signal[N,C], sampling_frequency)
 *     -> background_signal[N,C] float64                      (repet.py:67,205,422,571,712)
 * This header is what a ctypes binding of that call binds instead. Plain C types
 * only; the caller owns every buffer; the library keeps no caller pointer after a call returns.
 *
 * Every derived size (window length, period range in frames, cutoff bin, buffer length ...) crosses
 * the ABI as an INTEGER already evaluated by the caller with the reference's own expressions
 * (Python round()/np.round are half-to-even, C round() is not) -- the C side never converts
 * seconds to frames.
 *
 * Return value: 0 on success, negative repet_status otherwise; text via repet_last_error().
 * Thread-safety: a repet_ctx serialises its own calls on one HIP stream; different contexts may be
 * used from different host threads concurrently.
 */
#ifndef REPET_HIP_H
#define REPET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define REPET_ABI_VERSION 4

typedef enum repet_status {
    REPET_OK = 0,
    REPET_ERR_BAD_ARG = -1,   /* malformed argument: the Python shim raises ValueError            */
    REPET_ERR_TOO_SHORT = -2, /* clip too short for the algorithm (repet.py:1263, :802): ValueError */
    REPET_ERR_HIP = -3,       /* HIP runtime error: RuntimeError                                   */
    REPET_ERR_OOM = -4,       /* device allocation failed                                          */
    REPET_ERR_LIMIT = -5      /* size outside what the kernels support (documented in DESIGN.md)   */
} repet_status;

/* Which public function of the reference to run. */
typedef enum repet_algo {
    REPET_ORIGINAL = 0,  /* repet.py:67-202  */
    REPET_EXTENDED = 1,  /* repet.py:205-419 */
    REPET_ADAPTIVE = 2,  /* repet.py:422-568 */
    REPET_SIM = 3,       /* repet.py:571-709 */
    REPET_SIMONLINE = 4  /* repet.py:712-911 */
} repet_algo;

/* REPET_F16 / REPET_BF16: the device-side entries only (repet_ctx_upload_device_strided, repet_run_device); the host entries
 * refuse them.
 * As a DESTINATION dtype of a device-side entry (repet_ctx_download_device_strided, out_dtype of repet_run_device, dst_dtype of
 * the repet_online_*_device calls, repet_online_also_emit armed for one) each of the five is the inverse of the same source
 * dtype: a cast of the float64 value the engine holds, never a rescale. REPET_I16 ingest is the raw (float) cast, so REPET_I16
 * egress returns the same units (a +-1.0 float stream emitted as int16 is 0 / +-1): round to nearest, ties to even, saturated
 * to [-32768, 32767], NaN 0. REPET_F16 / REPET_BF16: the nearest value of the format, ties to even, rounded ONCE from float64
 * (not through float32): +-inf beyond the largest finite, subnormals produced, NaN stays NaN, the sign of zero is kept. The
 * host-array results stay float64. */
typedef enum repet_dtype { REPET_F32 = 0, REPET_F64 = 1, REPET_I16 = 2, REPET_F16 = 3, REPET_BF16 = 4 } repet_dtype;
/* (still ABI 4: an addition -- look the symbol up to detect it) 1 where `dtype` is a destination dtype of the device-side
 * entries (the five codes above), 0 for anything else. Touches no device. A library without this symbol writes REPET_F64 and
 * REPET_F32 only. */
int repet_emit_dtype_supported(int dtype);

/* The reference's nine module globals (repet.py:42-63), already converted to frames/bins/samples. */
typedef struct repet_params {
    int32_t window_length;       /* W = 2^ceil(log2(0.04 fs))                       repet.py:130 */
    int32_t step_length;         /* H = W/2                                         repet.py:132 */
    int32_t period_lo;           /* np.round(period_range[0]*fs/H)                  repet.py:165 */
    int32_t period_hi;           /* np.round(period_range[1]*fs/H)                  repet.py:165 */
    int32_t cutoff_bins;         /* round(cutoff_frequency*W/fs)                    repet.py:173 */
    int32_t filter_order;        /* adaptive median order                           repet.py:54  */
    int32_t seg_len_frames;      /* int(round(segment_length*fs/H))   (adaptive)    repet.py:519 */
    int32_t seg_step_frames;     /* int(round(segment_step*fs/H))     (adaptive)    repet.py:520 */
    int32_t sim_distance_frames; /* int(round(similarity_distance*fs/H))            repet.py:670 */
    int32_t sim_number;          /* similarity_number                               repet.py:60  */
    int32_t buffer_frames;       /* round(buffer_length*fs/H)         (simonline)   repet.py:787 */
    int32_t flags;               /* REPET_FLAG_* (0: the defaults); was reserved0 before ABI 3 */
    int64_t seg_len_samples;     /* round(segment_length*fs)          (extended)    repet.py:266 */
    int64_t seg_step_samples;    /* round(segment_step*fs)            (extended)    repet.py:267 */
    double sim_threshold;        /* similarity_threshold                            repet.py:58  */
} repet_params;

/* repet_params.flags -- samples that are not finite. repet.py never looks at its input (:125, :1220): a NaN sample makes the
 * frames that hold it NaN; `sim` / `simonline` confine the damage to those frames; the period family turns the beat spectrum
 * of the clip / segment / windows NaN (period = period_range[0] + 1 there) and, through np.median's NaN rule, marks the same
 * position of EVERY period. Since ABI 4 that is the DEFAULT here too (flags = 0, a fresh context): repet_run / repet_run_batch
 * (both transports) and the context calls let the samples through and all five variants return what the reference returns for
 * NaN samples: NaN positions equal, every other sample within the usual bar, periods and similar-frame lists equal (tested
 * against the oracle, which equals the reference bit for bit on such input). An INFINITE sample is treated as a NaN sample:
 * for `sim` / `simonline` that is the reference's result; for the period family the reference's own result depends on where
 * pocketfft's butterflies meet inf - inf, and the engine's NaN samples are a superset of the reference's.
 * REPET_FLAG_REFUSE_NONFINITE (bit 1) is the option: host arrays with such samples are refused (REPET_ERR_BAD_ARG, "contains
 * NaN or infinite samples" -- the default before ABI 4). Bit 0 (REPET_FLAG_STRICT_REFERENCE, the ABI-3 opt-in) is still
 * accepted and means the default. Any other bit is an argument error. Context calls: repet_ctx_set_strict_reference(ctx, 0)
 * turns the refusal on for that context's uploads. */
#define REPET_FLAG_STRICT_REFERENCE 1
#define REPET_FLAG_REFUSE_NONFINITE 2

/* repet_params.flags -- frames of digital silence in REPET_SIMONLINE (a muted microphone, a decoder that writes exact zeros,
 * the lead-in of a file). The reference divides such a frame's mean magnitude row by its norm, 0 / 0 (repet.py:1240): the unit
 * row is NaN, no comparison with it holds (repet.py:1318-1326), the frame's own list is empty, np.median of the empty list is
 * NaN, and the samples the frame covers are NaN; while the frame sits in the buffer its NaN column also keeps every frame
 * within similarity_distance of it out of all lists. That is the default here as well (flags without the bit), bit for bit.
 * REPET_FLAG_SILENT_FRAMES_ZERO (bit 2) is the option, for REPET_SIMONLINE only: through repet_run, repet_ctx_execute(_async),
 * batch contexts, repet_run_device, and repet_online_open / repet_online_open_streams, which keep `params`. A frame is SILENT
 * when the fp32 norm the forward STFT computes for its channel-mean magnitude row is exactly 0: exact-zero input gives that, and
 * so do magnitudes below fp32's square underflow (about 4e-23); a frame with a NaN sample has a NaN norm, is not silent and
 * keeps the reference's behaviour. Under the option
 *   - the unit row of a silent frame is all zeros, so the similarity of every pair with a silent member -- the frame with
 *     itself included -- is 0, by definition, at both refinement levels of the peak picking;
 *   - a silent frame has no list (count 0) and is in no other frame's list (with sim_distance_frames >= 1 and at least two
 *     columns that is what the reference's rule gives on the vector with zeros in the silent columns: a zero is never
 *     strictly above its neighbours);
 *   - a silent frame's masked spectrum is zero in every channel: it adds 0 to the overlap-add, and the frames around it ring
 *     into its samples as usual;
 *   - every other frame is the reference's, decided on a similarity vector whose silent columns are 0.
 * A frame whose list is empty for another reason (a NaN sample, an exact tie) stays NaN as before. What follows for a live
 * handle: last_frames of a silent frame is 0 in mixture, background and foreground; last_matches gives count 0, ages -1,
 * similarities 0 there; last_levels is finite; the background shaped by band gains is 0 there; every egress dtype, hold, feed /
 * tick, restart, export / import and start_frames keep their contracts (idle, held and pre-start rows are excluded by the
 * slot's origin as before). A clip without a silent frame gives the same bits with and without the bit. The other four
 * variants refuse the bit (REPET_ERR_BAD_ARG): original / extended / adaptive compute no similarity, and `sim` under the rule is
 * not built yet. The stream-state header carries `flags`, so a stream cannot move between a handle with the bit and one
 * without. REPET_ABI_VERSION stays 4; repet_silent_frames_supported() says that the bit is known. */
#define REPET_FLAG_SILENT_FRAMES_ZERO 4
int repet_silent_frames_supported(void);   /* 1. A library without this symbol refuses the bit as unknown. */

/* The nine module-level parameters of the reference (repet.py:42-63), for hosts that do not keep them as Python
 * globals, and the derivation of repet_params from them exactly as the reference's public functions do it
 * (Python round / np.round are half-to-even; so is this). repet_default_settings writes the reference's defaults:
 * 100 Hz, [1, 10] s, 10 s / 5 s segments, order 5, threshold 0, distance 1 s, 100 frames, 10-s buffer. */
typedef struct repet_settings {
    double cutoff_frequency;      /* Hz  */
    double period_range[2];       /* s   */
    double segment_length;        /* s   */
    double segment_step;          /* s   */
    double similarity_threshold;  /* [0, 1] */
    double similarity_distance;   /* s   */
    double buffer_length;         /* s   */
    int32_t filter_order;
    int32_t similarity_number;
} repet_settings;
void repet_default_settings(repet_settings* s);
int repet_derive_params(const repet_settings* s /* NULL: the defaults */, double sampling_frequency, repet_params* out);

/* Per-stage device time of the last repet_ctx_execute, from HIP events on the context's stream. */
#define REPET_MAX_STAGES 16
typedef struct repet_timing {
    int32_t n_stages;
    int32_t reserved0;
    float total_ms;                       /* first event to last event                     */
    float stage_ms[REPET_MAX_STAGES];     /* one entry per stage, in launch order          */
    char stage_name[REPET_MAX_STAGES][24];
    double stage_bytes[REPET_MAX_STAGES]; /* algorithmic HBM bytes of the stage */
    double stage_flops[REPET_MAX_STAGES]; /* algorithmic flops of the stage                 */
} repet_timing;

typedef struct repet_ctx repet_ctx;

/* ---- library --------------------------------------------------------------------------------- */
int repet_abi_version(void);
int repet_device_count(void);
/* (ABI 3) The CPUs of the NUMA node `device` hangs off, among those this process may run on (from the device's PCI address in
 * sysfs; *n_cpus = 0: unknown, or the machine has one node). On a two-socket host the drop-in call -- whose cost is host
 * threads narrowing the caller's array into pinned memory and two PCIe copies -- takes 3.9 ms when the calling process runs
 * on the GPU's node and 4.3 .. 5.9 ms elsewhere (180-s stereo clip): a host binds itself with
 * sched_setaffinity to these CPUs (repet.bind_host_to_device). The library pins only its OWN worker threads
 * (REPET_HOST_NUMA=0: not even those). */
int repet_device_host_cpus(int device, int32_t* cpus, int32_t capacity, int32_t* n_cpus);
const char* repet_last_error(void); /* thread-local text of the last failure on this thread */

/* ---- context: one per (host thread, device); owns a stream, workspaces, twiddle tables ------- */
int repet_ctx_create(int device, repet_ctx** out);
int repet_ctx_destroy(repet_ctx* ctx);

/* Device-resident path (what bench.py times): upload once, execute any number of times, download.
 * upload  : audio[n_samples*n_channels] in NumPy C order (audio[n*C + c]), converted to fp32 on device
 * execute : runs the whole algorithm on the resident clip; blocks until the stream is idle
 * download: background_signal as float64 [n_samples][n_channels]                                  */
int repet_ctx_upload(repet_ctx* ctx, const void* audio, int dtype, int64_t n_samples, int32_t n_channels);
/* n_clips equal-shape clips back to back, audio[n_clips][n_samples][n_channels] (a Python loop over
 * repet.simonline(clip, fs), BASELINE.json configs[4]). execute then separates every clip: simonline runs each
 * stage ONCE over all clips (one launch per stage instead of one per clip and stage), the other variants work
 * through the resident clips one after the other (repet_ctx_last_clip_passes tells which way a run went). download /
 * download_foreground return [n_clips][n_samples][n_channels]; the integer intermediates of a variant that works through the
 * clips are those of the last clip. */
int repet_ctx_upload_batch(repet_ctx* ctx, const void* audio, int dtype, int64_t n_samples, int32_t n_channels,
                           int32_t n_clips);
int repet_ctx_execute(repet_ctx* ctx, int algo, const repet_params* p, repet_timing* timing /* nullable */);
int repet_ctx_download(repet_ctx* ctx, double* out);

/* Device-resident ingest / egress (multi-GPU: a waveform received over RCCL/xGMI lands in device memory and goes
 * straight into the engine, no host bounce -- SURVEY 8e; the reference has no counterpart, its arrays live in host RAM):
 * fp32 interleaved [n_clips][n_samples][n_channels], device (or peer-accessible) memory, complete on return (the
 * producer of dev_audio must have finished; dev_out may be handed to a collective right away). */
int repet_ctx_upload_device(repet_ctx* ctx, const float* dev_audio, int64_t n_samples, int32_t n_channels, int32_t n_clips);
/* (ABI 2) The same with the fp32 REMAINDERS of a float64 waveform beside its fp32 samples: dev_audio_lo[i] = (float)(x[i] -
 * (double)(float)x[i]) (nullable: none). repet.py computes in float64 throughout (:149, :1223, :1318-1326); the engine takes
 * the few float64 decisions of its peak picking from sample + remainder = 48 bits of the caller's double, and a waveform
 * that reaches a device over RCCL must carry them to be separated exactly as the same waveform passed to repet_run is. */
int repet_ctx_upload_device_split(repet_ctx* ctx, const float* dev_audio, const float* dev_audio_lo, int64_t n_samples,
                                  int32_t n_channels, int32_t n_clips);
int repet_ctx_download_device(repet_ctx* ctx, float* dev_out);
/* Device-resident caller buffers of any layout (torch tensors on a ROCm device, a C++ host's own buffers), ordered by events
 * on the caller's stream; neither call waits on the host. Element i of the source is src[b * strides[0] + n * strides[1] +
 * c * strides[2]] for clip b, sample n, channel c (ELEMENT strides, non-negative: channels-first views, step slices and batch
 * slices are read as they lie).
 * repet_ctx_upload_device_strided : the context's stream waits for what `wait_stream` (a hipStream_t; NULL: the null stream)
 *     has enqueued so far, then narrows the source (REPET_F64 / F32 / I16 / F16 / BF16) into the resident fp32 samples --
 *     and, for REPET_F64, their fp32 remainders (see repet_ctx_upload_device_split): the planes a host upload of the same
 *     values leaves, bit for bit. The context is left as repet_ctx_upload_device_split leaves it (the planes are not scanned).
 *     REPET_FLAG_REFUSE_NONFINITE (repet_ctx_set_strict_reference(ctx, 0)) is the one case that waits: the ingest notes a
 *     sample that is not finite and the call reads that note back (one host wait) to refuse such a clip as the host path does.
 * repet_ctx_download_device_strided : the result into `dst` (REPET_F64: (double)v; REPET_F32; or REPET_I16 / F16 / BF16, the
 *     value rounded once as repet_dtype describes) of shape
 *     [n_clips][n_samples][n_channels] with the given strides (elements must not overlap), enqueued on the context's stream
 *     behind what `signal_stream` has enqueued so far; `signal_stream` then waits for it, so the caller's next work on that
 *     stream sees the result. */
int repet_ctx_upload_device_strided(repet_ctx* ctx, const void* src, int dtype, int32_t n_clips, int64_t n_samples,
                                    int32_t n_channels, const int64_t strides[3], void* wait_stream);
int repet_ctx_download_device_strided(repet_ctx* ctx, void* dst, int dtype, const int64_t strides[3], void* signal_stream);
/* (an addition to ABI 4) A RAGGED batch: clips of unequal lengths in one padded buffer. repet_ctx_upload_device_ragged is
 * repet_ctx_upload_device_strided with a HOST array of n_clips lengths, each in [0, n_samples]: clip b is its first lengths[b]
 * samples, n_samples is the PITCH of the batch. The samples at and behind a clip's length are never loaded (they may hold NaN,
 * infinities or stale memory, and the note of REPET_FLAG_REFUSE_NONFINITE looks at live samples only); the resident planes
 * hold zeros there. The lengths belong to the resident batch and are cleared by every upload. Lengths that all equal
 * n_samples ARE repet_ctx_upload_device_strided: the same kernels, the same bits. At most 65535 clips.
 * With lengths set,
 *   repet_ctx_execute / _async   REPET_SIMONLINE still runs every stage once over all clips, at the frame count of the pitch,
 *                                plus one launch that clears the frames behind each clip's own last one in front of the inverse
 *                                STFT; every other variant -- REPET_ORIGINAL included, which gives up its batched form -- works
 *                                through the clips one by one at each clip's own length. A clip too short for the variant is
 *                                refused before anything is enqueued, with the one-clip call's code and text and the clip named
 *                                in front (repet_check_clip_lengths makes the same check without a context); a clip of no
 *                                samples is refused by every variant.
 *   repet_ctx_download_device_strided, repet_ctx_result_levels_device
 *                                clip b's values below lengths[b] are those of the one-clip call on its lengths[b] samples --
 *                                in every signal, dtype and gain, the level record bit for bit (REPET_LEVEL_LIVE is lengths[b]) --
 *                                and zero of the destination's type from there to the pitch; neither the result nor the input is
 *                                read there.
 *   repet_ctx_download, repet_ctx_download_device, repet_ctx_download_foreground   refuse (REPET_ERR_BAD_ARG): the feature is
 *                                the device path.
 *   repet_ctx_last_frame_count, repet_ctx_last_sim_indices   report the last clip of the loop; after REPET_SIMONLINE the PADDED
 *                                geometry (the frame count of the pitch; the lists of rows at and behind a clip's own last frame
 *                                are not the clip's).
 * repet_ctx_clip_lengths : the lengths of the resident batch (n_samples for every clip of an equal one), up to `capacity` of
 * them; n_written is the number of clips. */
int repet_ctx_upload_device_ragged(repet_ctx* ctx, const void* src, int dtype, int32_t n_clips, int64_t n_samples,
                                   int32_t n_channels, const int64_t strides[3], const int64_t* lengths, void* wait_stream);
int repet_ctx_clip_lengths(repet_ctx* ctx, int64_t* out, int32_t capacity, int32_t* n_written);
int repet_check_clip_lengths(int algo, const repet_params* params, int32_t start_frames /* 0: buffer_frames */,
                             const int64_t* lengths, int32_t n_clips);
/* (ABI 3) Borrowed views for a host that keeps the exchange on the device (one process per GPU, torch.distributed over
 * RCCL: repet/parallel.py). The pointers stay valid until the next upload of this context (a larger clip may move the
 * buffers); what a run writes into the result is ordered on the context's stream, which repet_ctx_stream hands out so that
 * the host can enqueue its sends, receives and adds BEHIND the run instead of waiting for it on the CPU.
 * repet_ctx_result_view : the fp32 result [n_clips][n_samples][n_channels] of the last run (what repet_ctx_download widens)
 * repet_ctx_input_view  : the resident fp32 samples and, when a float64 upload left any, their fp32 remainders (else NULL)
 * repet_ctx_download_from: n_values fp32 values from ANY device buffer of this context's device widened into a host float64
 *                         array through the context's pinned ring (the gather side of a scatter: results received from peers) */
int repet_ctx_set_strict_reference(repet_ctx* ctx, int on);   /* (ABI 3; on by default since ABI 4) on = 0: REPET_FLAG_REFUSE_NONFINITE for this context's uploads */
int repet_ctx_stream(repet_ctx* ctx, void** hip_stream);
int repet_ctx_result_view(repet_ctx* ctx, float** dev_out, int64_t* n_values /* nullable */);
int repet_ctx_input_view(repet_ctx* ctx, float** dev_audio, float** dev_audio_lo /* nullable */, int64_t* n_values /* nullable */);
int repet_ctx_download_from(repet_ctx* ctx, const float* dev_src, int64_t n_values, double* out);
/* Declare the resident samples to be [sample0, sample0 + n_samples) of a clip of n_total samples, for
 * repet_ctx_execute_extended_range: a rank of a multi-GPU `extended` then holds (and returns) only the samples its own
 * segments cover -- (count + 1) segment steps instead of the whole clip (repet.py:306-414 touches nothing else).
 * Cleared by every upload; (0, 0) clears it. */
int repet_ctx_set_window(repet_ctx* ctx, int64_t n_total, int64_t sample0);

/* ---- WAVE files either side of the path (wavread / wavwrite, repet.py:914-946; README.md:62-72) -------------------
 * repet_wav_parse      : header of a RIFF/WAVE file image (PCM 8/16/24/32-bit, IEEE float 32/64-bit, plain or
 *                        WAVE_FORMAT_EXTENSIBLE); REPET_ERR_BAD_ARG with a message for anything else.
 * repet_ctx_upload_wav : the file's samples become the resident clip: the RAW bytes cross PCIe (2-3 bytes per sample, not
 *                        8), are decoded on the device and normalised exactly as wavread does -- divided by
 *                        2^(8*itemsize-1) of the array scipy.io.wavfile.read returns (repet.py:929; 24-bit PCM counts
 *                        as int32, float files are divided as well).
 * repet_ctx_result_wav : image of the file wavwrite(background | audio - background, fs, file) writes for a float64
 *                        (dtype REPET_F64) or float32 (REPET_F32) array: IEEE-float WAVE, fmt + fact + data chunks.
 *                        which: 1 background, 2 foreground. capacity >= 58 + n_samples*n_channels*itemsize. */
typedef struct repet_wav_info {
    int32_t format;              /* 1 PCM, 3 IEEE float (the sub-format of an extensible header) */
    int32_t n_channels;
    int32_t sampling_frequency;
    int32_t bits_per_sample;
    int32_t bytes_per_sample;    /* container width: block_align / n_channels */
    int32_t reserved0;
    int64_t data_offset;         /* first byte of the samples in the file image */
    int64_t n_samples;           /* per channel */
} repet_wav_info;
int repet_wav_parse(const void* file_bytes, int64_t n_bytes, repet_wav_info* info);
int repet_ctx_upload_wav(repet_ctx* ctx, const void* file_bytes, int64_t n_bytes, repet_wav_info* info_out);
int repet_ctx_result_wav(repet_ctx* ctx, int which, int dtype, void* file_out, int64_t capacity, int64_t* n_written);
/* sampling frequency repet_ctx_result_wav writes into the header when the clip did not come from repet_ctx_upload_wav */
int repet_ctx_set_sampling_frequency(repet_ctx* ctx, int32_t sampling_frequency);

/* Pinned host buffers from a recycling pool, for results: repet_ctx_download / repet_run write into any memory, but a
 * buffer that is already faulted in and pinned takes the copy at link speed (a fresh malloc / np.empty of a 3-minute
 * clip page-faults 31 000 times on first touch). repet_host_free returns the buffer to the pool; NULL when the pool
 * declines (use ordinary memory then). The Python module wraps these as the NumPy arrays it returns
 * (the reference returns a fresh array per call, repet.py:176,302,540,683,829). */
void* repet_host_alloc(size_t bytes);
void repet_host_free(void* ptr);
/* Non-blocking form of execute: enqueues the whole run on the context's stream and returns; contexts have
 * their own streams, so runs of different contexts overlap on the device. Errors detected at enqueue time are
 * returned here, device-side failures by repet_ctx_synchronize (or the next blocking call). */
int repet_ctx_execute_async(repet_ctx* ctx, int algo, const repet_params* p);
int repet_ctx_synchronize(repet_ctx* ctx);
/* Per-stage device times of runs that are enqueued back to back (bench.py's timed region): between begin and end every
 * repet_ctx_execute_async of this context (the first n_steps of them) records its own block of HIP events on the
 * context's stream; end waits for the stream and returns the MEAN stage times over the runs made (names, bytes and
 * flops as repet_ctx_execute's timing gives them). No host synchronisation happens between the runs. */
int repet_ctx_timing_series_begin(repet_ctx* ctx, int32_t n_steps);
int repet_ctx_timing_series_end(repet_ctx* ctx, repet_timing* mean, int32_t* n_steps /* nullable */);

/* The steps either side of the path in every README example (README.md:64-98), kept on the device:
 * foreground_signal = audio_signal - background_signal (README.md:69) of the last run, float64 [n][C];
 * and the magnitude spectrogram abs(_stft(mean over channels of the signal)[0:F]) (README.md:79-81) of the
 * mixture (which = 0), the background (1) or the foreground (2) as spec[T][F] fp32, T = repet_frame_count(n, W, W/2, 1). */
int repet_ctx_download_foreground(repet_ctx* ctx, double* out);
int repet_ctx_spectrogram(repet_ctx* ctx, int which, int32_t window_length, float* spec_out, int64_t n_frames);

/* extended only (repet.py:205-419): the segment plan of an n_samples clip (repet.py:271-281), and a run
 * restricted to segments [first, first+n_segments). Contributions of the other segments stay zero, and
 * the cross-fade is linear in the segments, so the outputs of disjoint ranges (e.g. one range per GPU)
 * add up to the full result. */
int64_t repet_extended_segment_count(int64_t n_samples, const repet_params* p);
int repet_ctx_execute_extended_range(repet_ctx* ctx, const repet_params* p, int64_t first, int64_t n_segments,
                                     repet_timing* timing /* nullable */);
/* (ABI 3) The same enqueued on the context's stream without waiting for it (see repet_ctx_execute_async). */
int repet_ctx_execute_extended_range_async(repet_ctx* ctx, const repet_params* p, int64_t first, int64_t n_segments);

/* ---- one-shot drop-in: replaces repet.<algo>(audio_signal, fs) (repet.py:67,205,422,571,712) -- */
/* Measurement aid (bench.py's roofline): the median of a list of at most list_bound values is a compare-exchange
 * selection network evaluated per lane (np.median, repet.py:1535); *network_size = wires of the compiled network
 * (0: lists longer than 128 use bisection), *instructions = min/max instructions per evaluation. A NEGATIVE list_bound asks
 * about the bit-sliced selection (mask_bits.hip) for lists of at most -list_bound entries: *network_size = 0, *instructions =
 * boolean wave instructions per frame (all its cells) and code plane. */
int repet_median_network_info(int32_t list_bound, int32_t* network_size, int32_t* instructions);

/* repet_run keeps one context per calling thread and device (stream, tables, grow-only workspaces -- for `sim` the
 * T x T similarity matrix) so that repeated calls reuse them; it is destroyed when the thread exits. This releases the
 * calling thread's contexts now (e.g. after a one-off long clip). */
int repet_release_thread_ctx(void);
int repet_run(int algo, const void* audio, int dtype, int64_t n_samples, int32_t n_channels,
              const repet_params* p, double* out, int device, repet_timing* timing /* nullable */);
/* The device-side twin of repet_run, for a host that keeps its audio on the GPU and has a HIP stream of its own: the same
 * per-thread, per-device context; ingest (repet_ctx_upload_device_strided, waiting for `stream`), repet_ctx_execute_async and
 * egress into `dst` (out_dtype REPET_F64 / F32 / I16 / F16 / BF16, signalling `stream`), all ordered on `stream` without a host wait
 * (except for REPET_FLAG_REFUSE_NONFINITE, see above, and the one-time growth of workspaces on a new shape). */
int repet_run_device(int algo, const void* src, int dtype, int32_t n_clips, int64_t n_samples, int32_t n_channels,
                     const int64_t in_strides[3], void* dst, int out_dtype, const int64_t out_strides[3],
                     const repet_params* p, int device, void* stream);

/* Batch of independent clips dealt round-robin (longest first) over n_devices GPUs of this process: one host thread,
 * context and stream per device; every device uploads its own clips from the caller's arrays and downloads its own
 * results (each over its own PCIe link). REPET_LOGICAL_DEVICES=n (test switch) lets n_devices exceed the visible GPUs:
 * logical device d runs on physical device d % visible. */
int repet_run_batch(int algo, int32_t n_clips, const void* const* audio, int dtype,
                    const int64_t* n_samples, const int32_t* n_channels, const repet_params* p,
                    double* const* out, int32_t n_devices);
/* The same with the waveforms travelling over xGMI: the clips enter through device 0 and are worked through in
 * rounds of one clip per device -- a round goes to its devices as ONE group of ncclSend / ncclRecv (fp32, interleaved; a
 * float64 clip as two planes, samples and remainders; ncclCommInitAll over devices 0 .. n_devices-1, cached; librccl opened
 * on first use), is separated from the received device buffers while the root stages the next round, and its results
 * return in a group of their own.
 * REPET_RCCL_SELF=1 with n_devices == 1 (test switch): every clip is sent by device 0 to itself inside the group.
 * repet_last_batch_info: what the calling thread's last batch call did -- out[0] transport (0 host, 1 RCCL), out[1] clips that
 * went through send / receive, out[2] clips whose remainder plane was resident when they were separated, out[3] RCCL groups
 * completed. */
int repet_last_batch_info(int64_t out[4]);
/* The resident clip as the engine holds it: the fp32 samples and, for a float64 upload, their fp32 remainders
 * (x - (double)(float)x; zeros and *has_remainders = 0 when none was needed). [n_clips][n_samples][n_channels] floats each. */
int repet_ctx_download_input(repet_ctx* ctx, float* samples_out, float* remainders_out, int32_t* has_remainders);
/* (ABI 4) Clips one after another through ONE device with `depth` (1 .. 8) of them in flight: every clip in flight has a
 * context of its own (stream, pinned ring, workspaces), so clip k + 1 is narrowed and uploaded and clip k - 1 copied back and
 * widened while clip k is separated. Results are what repet_run gives for each clip, bit for bit. The contexts stay cached
 * for the next call; repet_release_thread_ctx frees them. (What a root rank does with its own share of a scattered batch,
 * and the one-GPU form of repet.run_batch.) */
int repet_run_stream(int algo, int32_t n_clips, const void* const* audio, int dtype,
                     const int64_t* n_samples, const int32_t* n_channels, const repet_params* p,
                     double* const* out, int device, int32_t depth);
int repet_run_batch_rccl(int algo, int32_t n_clips, const void* const* audio, int dtype,
                         const int64_t* n_samples, const int32_t* n_channels, const repet_params* p,
                         double* const* out, int32_t n_devices);

/* ---- stage-level exports (parity tests; layouts follow the reference helper they replace) ---- */

/* repet.py:1021-1028 (centred=1) / repet.py:781 (centred=0): number of frames for n samples. */
int64_t repet_frame_count(int64_t n_samples, int32_t window_length, int32_t step_length, int32_t centred);

/* _stft, repet.py:1001-1060. x[n] one channel -> spec[T][F] interleaved (re,im) fp32, F = W/2+1
 * (frame-major; the reference's (W,T) array is its transpose plus the mirrored bins). */
int repet_stft(repet_ctx* ctx, const float* x, int64_t n, const float* window, int32_t window_length,
               int32_t step_length, int32_t centred, float* spec_out, int64_t n_frames);

/* _istft, repet.py:1063-1105. spec[T][F] (re,im) -> y[(T-1)*H] (centred: trimmed W-H each end and
 * divided by sum(window[0:W:H])). */
int repet_istft(repet_ctx* ctx, const float* spec, int64_t n_frames, const float* window,
                int32_t window_length, int32_t step_length, float* y_out, int64_t n_out);

/* _selfsimilaritymatrix, repet.py:1209-1225. v[T][F] (frame-major magnitudes) -> s[T][T]. */
int repet_selfsim(repet_ctx* ctx, const float* v, int64_t n_frames, int32_t n_freq, float* s_out);
/* The same with the SEGMENT RECORDS the peak picking of `sim` takes its candidates from (repet.py:1294-1345 scans every element;
 * a strict maximum of a window of +-d >= 31 elements is the maximum of its aligned 32-element segment): for every row and every
 * run of columns [32 u, 32 u + 32) the largest value (NaN counted as +inf), the largest of the run's OTHER elements (-inf for
 * a run of one), and the offset of the largest inside the run (the lowest among equals). max_out / second_out / at_out:
 * [n_frames][ceil(n_frames / 32)]. */
int repet_selfsim_records(repet_ctx* ctx, const float* v, int64_t n_frames, int32_t n_freq, float* s_out, float* max_out,
                          float* second_out, int32_t* at_out);
/* (still ABI 4: an addition -- look the symbol up to detect it) The similarity-matrix KERNELS as `sim` launches them, for tests:
 * rows[n_frames][n_freq] are taken as UNIT rows as they are (normalise != 0: made unit rows first, vn_out[Tpad][FS] brings them
 * back), with Tpad = round_up(n_frames, 128), FS = round_up(n_freq, 32), TS = round_up(n_frames, 64).
 *   form     0 what `sim` picks for n_frames, 1 fp32, 2 f16-split 128 x 128 tiles, 3 f16-split 256 x 256 tiles (2 and 3 at any
 *            n_frames >= 1);
 *   records  0 none, 1 as `sim` gets them (form 3: the kernel's epilogue, else a pass over S), 2 always by the pass over S;
 *   prefill  the byte every device buffer of the call holds before anything runs.
 * geo_out[8] = Tpad, FS, TS, seg_pitch, the form that ran, the records' source (0 none, 1 epilogue, 2 pass), the padded length
 * of the tile list, the tile edge. s_out == NULL: nothing runs, geo_out says what would (size the arrays from it). s_out[n_frames]
 * [TS] is the whole pitched image; max_out / second_out / at_out [n_frames][seg_pitch] (records != 0); planes_out
 * [round_up(n_frames, tile edge)][2 FS] f16 halves, per 32 bins [hi 32 | lo 32] (forms 2 and 3); kernel_out: the kernel's name.
 * REPET_ERR_BAD_ARG: a null argument, n_frames < 1, n_freq < 1, form or records out of range. REPET_ERR_LIMIT: n_frames > 4096
 * or n_freq > 8192. */
int repet_debug_gram_full_stage(repet_ctx* ctx, const float* rows, int64_t n_frames, int32_t n_freq, int32_t form, int32_t records,
                                int32_t normalise, int32_t prefill, int64_t* geo_out, float* s_out, float* max_out, float* second_out,
                                int32_t* at_out, uint16_t* planes_out, float* vn_out, char* kernel_out, int32_t kernel_cap);

/* _similaritymatrix, repet.py:1228-1246 (the online variant's frame-vs-buffer similarity):
 * a[TA][F], b[TB][F] frame-major magnitudes -> s[TA][TB] cosine similarities. */
int repet_similarity(repet_ctx* ctx, const float* a, int64_t n_a, const float* b, int64_t n_b, int32_t n_freq,
                     float* s_out);

/* _acorr, repet.py:1108-1139: x[n_rows][n_cols] -> unbiased autocorrelation of every column, ac[lag][col]. */
int repet_acorr(repet_ctx* ctx, const float* x, int32_t n_rows, int32_t n_cols, float* ac_out);

/* _beatspectrum, repet.py:1142-1158 (input already squared by the caller, as in the reference):
 * p[T][F] -> beat[n_lags], n_lags <= T. */
int repet_beat_spectrum(repet_ctx* ctx, const float* p, int64_t n_frames, int32_t n_freq,
                        float* beat_out, int32_t n_lags);

/* _beatspectrogram, repet.py:1161-1206: p[T][F] -> beat[T][seg_len] (frame-major). */
int repet_beat_spectrogram(repet_ctx* ctx, const float* p, int64_t n_frames, int32_t n_freq,
                           int32_t seg_len, int32_t seg_step, float* beat_out);

/* _periods, repet.py:1249-1291: beat[n_cols][n_lags] -> period[n_cols]. */
int repet_periods(repet_ctx* ctx, const float* beat, int32_t n_cols, int32_t n_lags, int32_t period_lo,
                  int32_t period_hi, int32_t* period_out);

/* _localmaxima over every row of m[n_rows][n_cols], repet.py:1294-1383: idx[n_rows][number] (-1 padded,
 * sorted by value descending) and count[n_rows]. */
int repet_local_maxima(repet_ctx* ctx, const float* m, int32_t n_rows, int32_t n_cols, float min_value,
                       int32_t min_distance, int32_t number, int32_t* idx_out, int32_t* count_out);

/* _mask / _adaptivemask / _simmask, repet.py:1386-1545: v[T][F] -> mask[T][F] (no high-pass override). */
int repet_mask_period(repet_ctx* ctx, const float* v, int64_t n_frames, int32_t n_freq, int32_t period,
                      float* mask_out);
int repet_mask_adaptive(repet_ctx* ctx, const float* v, int64_t n_frames, int32_t n_freq,
                        const int32_t* periods, int32_t filter_order, float* mask_out);
int repet_mask_sim(repet_ctx* ctx, const float* v, int64_t n_frames, int32_t n_freq, const int32_t* idx,
                   const int32_t* count, int32_t number, float* mask_out);

/* repet_mask_sim through the rank transform below (what `sim` does on clips of more than 1 024 frames): path 1 = the packed
 * 16-bit selection network on the rank codes, path 2 = the bit-sliced selection on the same codes; both give the bits of
 * repet_mask_sim. n_freq - 1 a multiple of 128 (path 2: a power of two <= 2048), lists of at most 128 entries.
 * median_codes_out (nullable, path 2): out[n_frames][n_freq - 1] as repet_ctx_last_median_codes describes them. */
int repet_mask_sim_ranked(repet_ctx* ctx, const float* v, int64_t n_frames, int32_t n_freq, const int32_t* idx,
                          const int32_t* count, int32_t number, int32_t path, float* mask_out, uint32_t* median_codes_out);

/* Rank transform behind the median of `sim` (np.median over the similar frames is a selection, repet.py:1535: it only
 * needs the ORDER of a bin's magnitudes over the clip). v[T][F] -> codes_out[T][n] (0x0400 + number of frames whose
 * magnitude in that bin is strictly smaller) and sorted_out[n][T] (every bin's magnitudes in ascending order), for the
 * first n = F rounded down to a multiple of 128 bins; 1024 < n_frames <= 30720. */
int repet_rank_columns(repet_ctx* ctx, const float* v, int64_t n_frames, int32_t n_freq, uint16_t* codes_out,
                       float* sorted_out);

/* Integer intermediates of the last repet_ctx_execute (for index-set / period parity checks).
 * periods: original -> 1 value; extended -> one per segment; adaptive -> one per frame.
 * sim indices: idx[T][number] (-1 padded) + count[T]; simonline: rows for frames B-1..T-1, FRAME numbers
 * (of a batch context: n_rows = rows of one clip gives the first clip's, rows * n_clips all clips' back to back). */
int repet_ctx_last_periods(repet_ctx* ctx, int32_t* out, int32_t capacity, int32_t* n_written);
int repet_ctx_last_sim_indices(repet_ctx* ctx, int32_t* idx_out, int32_t* count_out, int32_t n_rows,
                               int32_t number);
int repet_ctx_last_frame_count(repet_ctx* ctx, int64_t* n_frames);
/* The lists of clip `clip` of a batch context whose last run kept every clip's (REPET_SIMONLINE over a batch): n_rows = the
 * rows of one clip. clip 0 is repet_ctx_last_sim_indices itself, argument for argument (n_rows may also be the rows of all
 * clips): after a run that worked through the clips one after the other, and after a single clip, it is the only clip
 * accepted, and the lists are the last clip's. REPET_ERR_BAD_ARG for a clip the lists do not hold. */
int repet_ctx_last_sim_indices_clip(repet_ctx* ctx, int32_t clip, int32_t* idx_out, int32_t* count_out, int32_t n_rows,
                                    int32_t number);
/* How often the last repet_ctx_execute / _async enqueued its variant's pipeline: 1 for a single clip and for a batch that
 * went through every stage together (REPET_SIMONLINE, REPET_ORIGINAL over equal clips), n_clips for a variant, or a ragged
 * batch, that works through the clips one after the other. 0 before the first run. Detect the entry point by its symbol; the
 * ABI version is unchanged. */
int repet_ctx_last_clip_passes(repet_ctx* ctx, int32_t* passes);
/* sim: which form of np.median (repet.py:1535) the last run took -- 0 the selection network on the float magnitudes,
 * 1 the packed 16-bit network on the rank codes (rank.hip), 2 the bit-sliced selection on the same codes (mask_bits.hip).
 * All three give the same bits; REPET_MEDIAN=f32|rank forces the first two. */
int repet_ctx_last_median_path(repet_ctx* ctx, int32_t* path);
/* After a run on path 2: what the selection left per cell, out[channel][frame][bin] for the first n_bins bins (n_bins <=
 * n_freq - 1: the Nyquist bin is not ranked): bits 0-14 the rank code (number of strictly smaller magnitudes of the bin over
 * the clip, rank.hip, without its 0x0400 base) of the lower median of the frame's similar frames, bit 15 set where that is
 * below the frame's own code, bits 16-30 the code of the upper median (equal to the lower one for an odd list).
 * Bin 1 is the exception when the high-pass cutoff covers at least one bin (cutoff_bins >= 1, the default): its mask is 1
 * whatever its median, so its column of the rank transform carries the Nyquist bin instead, and the words at bin 1 are
 * those of bin n_freq - 1 -- codes among the Nyquist magnitudes, the flag against the frame's own Nyquist code.
 * (REPET_NYQUIST_COLUMN=0, or a cutoff of 0 bins: bin 1's own.) */
int repet_ctx_last_median_codes(repet_ctx* ctx, uint32_t* out, int64_t n_frames, int32_t n_bins);
/* sim / simonline: counters of the near-tie refinement of the last run's peak picking (_localmaxima,
 * repet.py:1294-1345): out[0] rows with a decision inside the fp32 tolerance, out[1] near-tied elements
 * re-decided from float64 similarities, out[2] decisions that changed, out[3] flat rows left to fp32. */
int repet_ctx_last_refine_stats(repet_ctx* ctx, int64_t out[4]);
/* The second level of the same peak picking: the reference decides on float64 similarities of complex128 spectra
 * (repet.py:149, :1220-1223, :1318-1326). Rows whose float64 re-decision on the fp32 spectra met a comparison the fp32
 * spectra cannot settle (closer than 2.5e-7), and flat rows, are decided again from float64 spectra computed from the
 * waveform. out[0] rows decided again, out[1] elements given float64 spectra, out[2] rows whose list changed,
 * out[3] largest |fp32-spectra value - float64-spectra value| met, in units of 1e-12, out[4] float64 unit rows computed,
 * out[5] 1 when the resident clip carries the fp32 remainders of a float64 upload (48-bit samples), out[6] rows taken up
 * again from the first pass's records (the fast path), out[7] of those, rows handed on to the general path. */
int repet_ctx_last_exact_stats(repet_ctx* ctx, int64_t out[8]);

/* ---- streaming online REPET-SIM (the reference's simonline needs the whole signal, repet.py:712-911) ------
 * open  : state for one stream of n_channels (any number, as repet.py:812 loops) with the parameters of derive_params(fs);
 * push  : feed n_samples more samples (NumPy C order); every frame that is now complete is processed and the
 *         newly final background samples (whole hops of W/2) are written to out (float64, interleaved,
 *         `capacity` samples per channel; n_samples + window_length always suffices), their count to *n_written;
 * finish: end of stream -- the zero-padded last frame (repet.py:781,813) and the tail; afterwards the total
 *         written equals the total pushed. REPET_ERR_TOO_SHORT if fewer samples were pushed than the reference's
 *         warm-up needs (repet.py:795-810).
 * The concatenated output equals repet.simonline(whole signal) bit for bit (same kernels, same order). */
typedef struct repet_online repet_online;
int repet_online_open(int device, int32_t n_channels, const repet_params* p, repet_online** out);
int repet_online_push(repet_online* h, const void* audio, int dtype, int64_t n_samples, double* out, int64_t capacity,
                      int64_t* n_written);
int repet_online_finish(repet_online* h, double* out, int64_t capacity, int64_t* n_written);
int repet_online_close(repet_online* h);

/* (ABI 4 additions) S live streams of one sampling frequency and channel count in ONE handle, in lockstep: every push brings
 * the same number of samples n for every stream, so all the counters are shared and only the data is per stream. A push
 * enqueues one fixed sequence of launches for all S streams (its length depends on neither S nor C). Each stream's
 * concatenated output equals repet.simonline of that stream's concatenated input, bit for bit; repet_online_open / push /
 * finish above are the S = 1 case of the same engine. Samples that are not finite are let through (REPET_FLAG_REFUSE_NONFINITE
 * is not honoured here). Host and device pushes may be mixed on one handle.
 * open_streams : max_push_samples sizes the sliding windows and the pending buffers at open (0: they grow on demand). A
 *                device push of at most that many samples never waits on the host once the per-push workspaces have seen
 *                a push of its size; a larger one may grow the buffers and wait for the device once.
 * emit_count   : samples per stream that the next push of n samples (finishing = 0) or the finish (finishing = 1) will write:
 *                full = (total - W) / H + 1 frames are complete once total >= W samples were pushed, a push writes
 *                (full - frames done) * H, the finish the rest (REPET_ERR_TOO_SHORT, as repet_online_finish, before the
 *                buffer has filled).
 * push_streams : host chunk audio[S][n][C] (F32 / F64 / I16, C order) -> out[S][n_emit][C] float64 (capacity: samples per
 *                stream); returns once out is written. For S = 1 this is exactly repet_online_push.
 * push_device  : device chunk with element strides [stream, sample, channel] (F64 / F32 / I16 / F16 / BF16, as
 *                repet_ctx_upload_device_strided), read behind what wait_stream has enqueued; the result is widened into dst
 *                (F64 / F32, or I16 / F16 / BF16 rounded once as repet_dtype describes; element strides, elements must not
 *                overlap) and signal_stream is made to wait for it. No host wait. A 16-bit destination costs no launch more.
 * finish_*     : the end of every stream, to the host or into a device destination like push_device's. */
int repet_online_open_streams(int device, int32_t n_streams, int32_t n_channels, const repet_params* p,
                              int64_t max_push_samples, repet_online** out);
int repet_online_emit_count(repet_online* h, int64_t n, int finishing, int64_t* n_emit);
int repet_online_push_streams(repet_online* h, const void* audio, int dtype, int64_t n, double* out, int64_t capacity,
                              int64_t* n_written);
int repet_online_push_device(repet_online* h, const void* src, int dtype, int64_t n, const int64_t src_strides[3],
                             void* wait_stream, void* dst, int dst_dtype, const int64_t dst_strides[3], void* signal_stream,
                             int64_t* n_written);
int repet_online_finish_streams(repet_online* h, double* out, int64_t capacity, int64_t* n_written);
int repet_online_finish_device(repet_online* h, void* dst, int dst_dtype, const int64_t dst_strides[3], void* signal_stream,
                               int64_t* n_written);

/* (still ABI 4: additions only -- look the symbols up to detect them) Streams that join and leave ONE BY ONE. The S streams of
 * a handle are S slots. Pushes stay in lockstep ((S, n, C) in, (S, n_emit, C) out, n_emit as above); what is per slot is which
 * stream lives in it and since when. With P = samples per slot pushed so far, W the window, H = W / 2, B buffer_frames:
 * restart_streams : each named slot begins a new stream whose sample 0 is the handle's sample P. Only where P % H == 0
 *                   (REPET_ERR_BAD_ARG otherwise, nothing changes). What lived in the slot is discarded; the frame that
 *                   straddles P and everything older reach neither the new stream's similarity buffer nor its overlap-add
 *                   (NaN in them included). The slot's lockstep output from sample P on, followed by its finish_stream (or
 *                   finish) tail, equals repet.simonline of the new stream's samples, bit for bit: zeros while it is younger
 *                   than B - 1 frames, then its own B-frame buffer at circular positions (its own frame number) % B.
 * release_streams : the named slots become idle without output. An idle slot ignores what the lockstep chunk carries for it
 *                   (NaN included) and emits zeros.
 * stream_emit_count / finish_stream(_device): end the stream of ONE slot where the handle stands (any P, on the hop grid or not):
 *                   its zero-padded last frame and its tail of P - (samples emitted) samples, out[n][C] float64 on the host or
 *                   a device destination with element strides [sample, channel] as finish_device's. REPET_ERR_BAD_ARG for an
 *                   idle slot, REPET_ERR_TOO_SHORT for a stream shorter than (B - 2) H + W (the slot then stays as it was).
 *                   Touches no other slot and no counter of the handle; the slot is idle afterwards.
 * repet_online_finish_* keeps its meaning: it ends every live slot, each with its own length (a stream still younger than the
 * buffer has only zeros to give); idle slots return zeros. Every call enqueues on the handle's stream with no host wait (the
 * host forms of finish_stream wait for their result); restart / release are one launch per 256 slots named. A handle on which
 * none of these calls was made behaves exactly as before. */
int repet_online_restart_streams(repet_online* h, const int32_t* slots, int32_t n_slots);
int repet_online_release_streams(repet_online* h, const int32_t* slots, int32_t n_slots);
int repet_online_stream_emit_count(repet_online* h, int32_t slot, int64_t* n_emit);
int repet_online_finish_stream(repet_online* h, int32_t slot, double* out, int64_t capacity, int64_t* n_written);
int repet_online_finish_stream_device(repet_online* h, int32_t slot, void* dst, int dst_dtype, const int64_t dst_strides[2],
                                      void* signal_stream, int64_t* n_written);

/* (still ABI 4: additions only -- look the symbols up to detect them) A live stream MOVED between handles. A slot's stream is
 * its state -- the last B - 1 frames of magnitudes and unit rows, the overlap-add tail, the delay line of samples with their
 * fp32 remainders -- and export_stream copies that state out as a value: a small host-side header and a dense payload whose
 * size depends on W, H, B and the channel count alone. import_stream loads it into any slot of any handle opened with the same
 * parameters (same GPU, another GPU, another process, now or later), and the stream goes on bit for bit as if it had never
 * moved: what the exporting slot emitted before the export, then what the importing slot emits in lockstep, then its
 * finish_stream / finish tail, equal repet.simonline of the stream's whole input.
 * stream_state_size : bytes of the header (96) and of the payload for this handle's parameters.
 * export_stream(_device): a SNAPSHOT of `slot` -- the slot lives on untouched, last_emission stays valid; migration is export +
 *                   release_streams, and a snapshot may be imported any number of times (checkpoint, fork). Only where
 *                   P % H == 0 and the slot is live (REPET_ERR_BAD_ARG otherwise). One launch gathers the slot's share of
 *                   the handle's buffers; the host form returns once payload_out is written, the device form (payload_dev:
 *                   payload bytes of device memory on the handle's device) enqueues only and orders signal_stream behind it.
 *                   header_out is complete on return in both forms: the host knows it without touching the device.
 * import_stream(_device): drops what lived in `slot`, as restart_streams does, and loads the state; last_emission becomes
 *                   stale. Only where P % H == 0. REPET_ERR_BAD_ARG, before any launch, for a header with an unknown magic
 *                   word or version, with a geometry (W, H, B, C, F), a parameter (cutoff_bins, sim_distance_frames,
 *                   sim_number, sim_threshold, buffer_frames, flags) or a payload size other than the handle's, or with
 *                   counts that contradict each other. One launch scatters the payload and writes the slot's first frame,
 *                   which is the handle's next frame minus the stream's age: negative for a stream older than the handle.
 *                   A handle younger than the state needs (fewer frames done than the state has history rows) is first
 *                   read as if it had been opened that many hops earlier with every live slot idle until its own start
 *                   (one more launch moves the held samples; buffers may grow, which waits); what the caller pushed per
 *                   slot does not change, and every other slot's output is what it would have been (on a handle that has
 *                   seen fewer than ceil(W / H) - 1 hops, behind as many hops of zeros as it lacked: the state brings
 *                   samples that are held but not yet emitted, and emissions are in lockstep). The device form
 *                   starts behind what wait_stream has enqueued and orders wait_stream behind its read of payload_dev.
 * Header (little-endian, no padding): uint32 magic "REPS", uint32 version 1, int32 W, H, B, C, F, cutoff_bins,
 * sim_distance_frames, sim_number, buffer_frames, flags, double sim_threshold, int64 age in frames (length / H - (ceil(W / H)
 * - 1)), length in samples, valid history rows, pending samples, payload bytes. Payload (fp32, every part at a 16-byte
 * aligned offset, rows right-aligned and zero where the stream is younger): Vn [B-1][FS] | V [C][B-1][FS] | X [C][FS] complex
 * | samples [(B-1) H + (ceil(W / H) - 1) H][C] | their remainders likewise, FS = F rounded up to 32. */
int repet_online_stream_state_size(repet_online* h, int64_t* header_bytes, int64_t* payload_bytes);
int repet_online_export_stream(repet_online* h, int32_t slot, void* header_out, void* payload_out);
int repet_online_export_stream_device(repet_online* h, int32_t slot, void* header_out, void* payload_dev, void* signal_stream);
int repet_online_import_stream(repet_online* h, int32_t slot, const void* header, const void* payload);
int repet_online_import_stream_device(repet_online* h, int32_t slot, const void* header, const void* payload_dev,
                                      void* wait_stream);

/* (still ABI 4: additions only -- look the symbols up to detect them) Separation that STARTS BEFORE THE BUFFER IS FULL. The
 * reference writes nothing until its buffer holds B = buffer_frames frames (10 s at the defaults, repet.py:795-834) only because
 * its warm-up loop is written that way; what it does at its first processed frame is well defined on a buffer that is still
 * growing. With M = start_frames, 1 <= M <= B (M = B: the reference, the default everywhere), a stream's own frames j = 0, 1, ...:
 *   j < M - 1        : a warm-up frame as before -- mask 0, nothing added to the background, the foreground is the input;
 *   M - 1 <= j < B - 1 : a YOUNG frame. The buffer is the stream's own frames 0 .. j in columns 0 .. j (the circular position
 *                      equals the frame number while j < B). The similarity vector has j + 1 elements and
 *                      _localmaxima(vector, similarity_threshold, similarity_distance2, similarity_number) runs on exactly
 *                      those: the columns past j are ABSENT, not zero (repet.py:1322-1326 clips its windows at the vector's
 *                      ends). Median, np.minimum, mask, high-pass rule and overlap-add as in repet.py:869-898. Element for
 *                      element this is what the reference computes for its first processed frame when buffer_length2 == j + 1.
 *                      While j <= similarity_distance2 the frame's only similar frame is itself: its mask is 1, the whole
 *                      input counts as background and the foreground is silent -- a sensible M is two or three times
 *                      similarity_distance2 at least;
 *   j >= B - 1       : unchanged, bit for bit.
 * A stream is too short (REPET_ERR_TOO_SHORT of finish / finish_stream / execute) when it has fewer than (M - 2) H + W samples:
 * the rule above with M in place of B. emit_count and stream_emit_count do not change (the warm-up emits its hops as zeros
 * already), and a push enqueues the same launches whatever M is.
 * repet_online_set_start_frames : M of the handle, for every slot and every later restart. Only before the handle's first push
 *                   (REPET_ERR_BAD_ARG afterwards, and for a value outside [1, B]; nothing changes then).
 * repet_online_start_frames     : the handle's M.
 * repet_ctx_set_online_start    : M of REPET_SIMONLINE runs of this context alone (one clip or a batch); 0 = B, the reference.
 *                   Checked against B when the run executes (REPET_ERR_BAD_ARG for M > B). repet_ctx_last_sim_indices then
 *                   returns T - M + 1 rows, for frames M - 1 .. T - 1.
 * Migration: M belongs to the HANDLE, not to the stream. The 96-byte header and the payload are unchanged; export_stream of a young
 * stream works as for any other (the state holds right-aligned history rows, zero where the stream is younger), and an imported
 * stream goes on under the importing handle's M -- bit for bit where both handles have the same M. */
int repet_online_set_start_frames(repet_online* h, int32_t start_frames);
int repet_online_start_frames(repet_online* h, int32_t* out);
int repet_ctx_set_online_start(repet_ctx* ctx, int32_t start_frames);

/* (still ABI 4: additions only -- look the symbols up to detect them) The FOREGROUND, aligned. The repeating background is the
 * means; audio - background is what most callers want, and a live handle returns its background behind the input (n_emit != n),
 * so only the handle knows which input samples an emission belongs to. One selector with one meaning everywhere: */
#define REPET_OUT_BACKGROUND 0   /* what every call returned so far, bit for bit (the default) */
#define REPET_OUT_FOREGROUND 1   /* input - background of the same samples */
#define REPET_OUT_MIXTURE 2      /* the input samples themselves, aligned with what was emitted (the delay-compensated input) */
/* With x the sample as the engine holds it (fp32 sample + fp32 remainder: exact for F32 / F16 / BF16 / I16 input and for
 * float64 input that came from PCM or fp32, 48 bits of any other float64 sample) and bg the fp32 background: mixture =
 * (double)x, foreground = (double)x - (double)bg, rounded once; an F32 / I16 / F16 / BF16 destination takes that value rounded
 * once more (straight from float64: see repet_dtype). A sample
 * before its slot's own stream began (the hop emitted behind a restart, every sample of an idle slot) is zero in all three
 * signals, whatever the chunk carried there; from the slot's first own sample on, foreground and mixture are its input, the
 * warm-up included (the background is zero there: nothing is removed before there is evidence).
 * set_output       : what `out` / `dst` of every emitting call of the handle (push*, finish*, finish_stream*) carries from now on.
 * also_emit        : ONE-SHOT: the next emitting call also writes `which` of the same samples, in the same launch, into `dst`:
 *                    device memory of `dtype` (that call's dst_dtype) with element strides [stream, sample, channel] for the
 *                    *_device calls (finish_stream_device ignores the stream stride), a dense float64 host array [S][n_emit][C]
 *                    (dtype REPET_F64, strides ignored) for the host calls. The address ranges of the two destinations must
 *                    not intersect. Consumed by that call whether it succeeds or not; checked by it before any launch.
 * last_emission(_device): another signal of exactly the samples the last push or finish wrote -- out[S][n][C] float64 on the
 *                    host, or a device destination as push_device's behind `signal_stream`, with no host wait. Valid until the
 *                    next push, finish, restart or release on the handle (REPET_ERR_BAD_ARG afterwards: the handle no longer
 *                    holds those samples). A finish_stream releases its slot, so its tail is had through also_emit only.
 * No stage of the pipeline runs twice: the selected signal costs the launch the background's egress costs, a second one rides
 * in the same launch. Offline contexts: repet_ctx_select_result chooses what repet_ctx_download_device_strided writes from now
 * on (the resident samples and, after a float64 upload, their remainders against the result); repet_select_run_result does the
 * same for the calling thread's repet_run_device context of `device`. */
int repet_online_set_output(repet_online* h, int which);
int repet_online_also_emit(repet_online* h, int which, void* dst, int dtype, const int64_t strides[3]);
int repet_online_last_emission(repet_online* h, int which, double* out, int64_t capacity, int64_t* n_written);
int repet_online_last_emission_device(repet_online* h, int which, void* dst, int dst_dtype, const int64_t dst_strides[3],
                                      void* signal_stream, int64_t* n_written);
int repet_ctx_select_result(repet_ctx* ctx, int which);
int repet_select_run_result(int device, int which);

/* (still ABI 4: additions only -- look the symbols up to detect them) KEEP A CHOSEN SHARE OF THE BACKGROUND in the foreground.
 * Dialogue enhancement, ducking and karaoke attenuate the repeating background by some decibels instead of removing it. A
 * background gain g in [0, 1] changes what REPET_OUT_FOREGROUND means, wherever that selector already works (push*, finish*,
 * finish_stream*, last_emission*, the second destination of also_emit, host and device forms, F64 and F32 destinations):
 *     foreground = x - a * bg,   a = (float)(1.0 - (double)g)   (an fp32 value)
 * computed as fma(-a, bg, x) in float64 by the egress launch itself: a * bg is fp32 x fp32 and exact, so the foreground is
 * x - a * bg rounded once (an F32 destination rounds once more). g = 0, the default, is the foreground as it was, bit for bit
 * (-12 dB of background: g = pow(10, -12.0 / 20)); g = 1 returns the input, except where bg is NaN or infinite (0 * NaN). The
 * background and mixture signals, every counter and the exported stream state do not change; samples before a slot's own
 * stream began stay zero.
 * repet_online_set_background_gain : gains[k] for slots[k], k < n_slots; slots == NULL: gains[0] for every slot (n_slots is
 *                   ignored). A slot named twice takes the last value. REPET_ERR_BAD_ARG, before anything is enqueued and with
 *                   nothing changed, for a slot out of range or a gain that is NaN, infinite or outside [0, 1]. Enqueues only
 *                   (one small launch per 256 slots named), no host wait. The gain is the SLOT's setting, not the stream's: it
 *                   survives restart_streams, release_streams, finish_stream and import_stream, and it is not part of an
 *                   exported state. A CHANGE IS A FADE: the first emitting call that covers the slot after a set (every slot
 *                   for push* / finish*, the one slot for finish_stream*) moves a linearly from the value in force to the
 *                   new one over its first R = min(step_length, n_emit) samples -- sample k (0-based, per stream) takes
 *                   fma(a_new - a_old, (double)(k + 1) / R, a_old) in float64 for k + 1 < R and a_new itself from k + 1 == R
 *                   on -- so the fade is complete when that call returns; it costs that call one small launch more, and a
 *                   push in steady state enqueues exactly what it enqueued before. last_emission(REPET_OUT_FOREGROUND) returns
 *                   what the emission's own gain and fade produced, whatever was set since. Before the first set on a
 *                   handle no kernel is given a gain and everything is as it was.
 * repet_online_background_gain     : the g last set for `slot` (0 before any set), from the host's copy: no device work.
 * repet_ctx_set_background_gain    : g for the foreground repet_ctx_download_device_strided writes from now on (a scalar for
 *                   every clip, no fade); the same range rule. 0 restores the original path.
 * repet_set_run_background_gain    : the same for the calling thread's repet_run_device context of `device`, with the lifetime
 *                   repet_select_run_result has (the value is checked before a context is made). */
int repet_online_set_background_gain(repet_online* h, const int32_t* slots, int32_t n_slots, const float* gains);
int repet_online_background_gain(repet_online* h, int32_t slot, float* gain_out);
int repet_ctx_set_background_gain(repet_ctx* ctx, float gain);
int repet_set_run_background_gain(int device, float gain);

/* (still ABI 4: additions only -- look the symbols up to detect them) A share of the background kept BAND BY BAND, on the live
 * handles. Every slot has a table g[k], k < F = window_length / 2 + 1, every entry in [0, 1], all zero by default. With
 *     a[k] = (float)(1.0 - (double)g[k])
 * the SHAPED background of a slot is the handle's overlap-add inverse STFT with the masked spectrum Y_j of frame j taken as
 * a_j[k] * Y_j[k] (one fp32 rounding per product, bin N - k with bin k's factor; the same window sum and trimming), and the
 * foreground is fma(-a_s, shaped_bg, x) in float64, a_s the slot's scalar gain above with its fade: the two gains multiply.
 * The background, the mixture, last_frames in all three signals, the MIX / BG / LIVE / NONFINITE level fields, every counter
 * and the exported state do not change by a bit; FG_ENERGY / FG_PEAK measure the shaped foreground; idle and held slots and the
 * samples before a slot's stream began stay zero. g = 1 on every bin returns the input for finite input.
 * WHICH TABLE A FRAME GETS: frame j of a slot is shaped, once and whole, with the table the slot had when the push or finish
 * that completed frame j was enqueued. A frame overlap-adds into two hops, so a change cross-fades through the analysis window
 * over one frame; the frame carried over from the call before keeps the table it was completed under. A set on a held slot
 * applies to the frames completed after its resume. A frame that arrives with import_stream is shaped with the importing
 * slot's table. The table is the SLOT's: it survives restart_streams, release_streams, finish_stream and import_stream, and it
 * is not part of an exported state.
 * repet_online_set_background_band_gains : the tables of slots[k], k < n_slots (slots == NULL: every slot, n_slots ignored),
 *                   replaced whole. edges: n_bands + 1 ascending bins in [0, F], 1 <= n_bands <= F; band b is the bins
 *                   [edges[b], edges[b + 1]) and takes gains[r * n_bands + b], bins outside every band take 0. edges == NULL:
 *                   one gain per bin, n_bands == F. gains_rows is 1 (row r = 0 for every slot named) or the number of slots
 *                   named (r = k; a slot named twice takes the last row). REPET_ERR_BAD_ARG, before anything is enqueued and
 *                   with nothing changed, for a gain that is NaN or outside [0, 1], bad edges, a slot out of range or a wrong
 *                   size; REPET_ERR_LIMIT on a handle whose window_length exceeds 4096. At any time, on or off the hop grid:
 *                   one small launch, no host wait, and the last emission stays valid (it was shaped already).
 *                   COST: a handle on which no table was ever set enqueues what it always did. While any slot's table -- as
 *                   set, or as still in force for a frame -- is not all zero, every emitting call enqueues one inverse-STFT
 *                   launch more, and each of the first two frame-completing calls after a set one small launch that brings
 *                   the tables up to date. Two frame-completing pushes after every table was cleared the handle is back to
 *                   what it enqueued before.
 * repet_online_background_band_gains     : the F gains last set for `slot` (zeros before any set) into out (capacity >= F
 *                   floats), from the host's copy: no device work. */
int repet_online_set_background_band_gains(repet_online* h, const int32_t* slots, int32_t n_slots, const int32_t* edges, int32_t n_bands,
                                           const float* gains, int32_t gains_rows);
int repet_online_background_band_gains(repet_online* h, int32_t slot, float* out, int32_t capacity);

/* (still ABI 4: additions only -- look the symbols up to detect them) The same share of the background BAND BY BAND for the
 * TENSOR calls: a context (and the per-thread context of repet_run_device) keeps one table per clip for the whole clip -- the
 * statement above without the frame rule. With a[k] = (float)(1.0 - (double)g[k]) the SHAPED background of a clip is the
 * variant's own inverse STFT with the masked spectrum Y_j[k] = fl(m_j[k] * X_j[k]) taken as fl(a[k] * Y_j[k]) (two fp32
 * roundings per component, the first the plain path's; bin N - k with bin k's factor; the same overlap-add, window sum,
 * trimming and centring, and for `extended` the same triangular cross-fade of the segments), and the foreground is
 * fma(-a_s, shaped_bg, x) in float64, a_s from repet_ctx_set_background_gain: the two gains multiply. The background, the
 * mixture, the MIX / BG / LIVE / NONFINITE level fields, repet_ctx_download, repet_ctx_download_foreground,
 * repet_ctx_result_wav, repet_ctx_spectrogram, the similar-frame lists and the periods do not change by a bit; FG_ENERGY /
 * FG_PEAK measure the shaped foreground; g = 1 on every bin returns the input for finite input. A table that is all zero is
 * no table: the run enqueues the plain path and its foreground is the plain one bit for bit.
 * WHICH TABLE A RUN GETS: the one in force when repet_ctx_execute(_async) is enqueued. A set or clear afterwards changes the
 * next run; the result already made keeps its shaped background -- for repet_ctx_download_device_strided with
 * REPET_OUT_FOREGROUND and repet_ctx_result_levels_device, in all five destination dtypes -- until the next execute or upload.
 * COST: under a table every inverse-STFT launch of the variant is followed by one more, with the factor rows beside the mask
 * plane, the repeating-segment model or the masked-in-place spectrum the first one read, into a second result buffer that
 * exists only once a table was set. A context on which none was set enqueues what it always did.
 * repet_ctx_set_background_band_gains : edges and gains as for repet_online_set_background_band_gains, F from window_length.
 *                   gains_rows is 1, or the number of clips of the next upload (row b for clip b). gains == NULL or
 *                   n_bands == 0 clears. REPET_ERR_BAD_ARG, with nothing changed, for a gain that is NaN or outside [0, 1],
 *                   bad edges, a window_length that is no power of two in [64, 8192] or a wrong size; REPET_ERR_LIMIT for a
 *                   window_length above 4096 (its inverse kernel has no masked form). The factor rows are copied on the
 *                   context's stream, behind the runs enqueued so far, and the call waits for that copy.
 *                   An execute is refused with REPET_ERR_BAD_ARG before anything is enqueued when params->window_length is
 *                   not the table's, or gains_rows is neither 1 nor the number of resident clips;
 *                   repet_ctx_execute_extended_range(_async) is refused while a table that is not all zero is set (the
 *                   shards of a multi-GPU `extended` do not take one).
 * repet_ctx_background_band_gains     : the F gains of `clip` (any clip where one row was given) into out (capacity >= F
 *                   floats), from the host's copy: no device work. REPET_ERR_BAD_ARG when no table is set.
 * repet_set_run_background_band_gains : the same set or clear for the calling thread's repet_run_device context of `device`,
 *                   with the lifetime repet_set_run_background_gain has. */
int repet_ctx_set_background_band_gains(repet_ctx* ctx, int32_t window_length, const int32_t* edges, int32_t n_bands,
                                        const float* gains, int32_t gains_rows);
int repet_ctx_background_band_gains(repet_ctx* ctx, int32_t clip, float* out, int32_t capacity);
int repet_set_run_background_band_gains(int device, int32_t window_length, const int32_t* edges, int32_t n_bands,
                                        const float* gains, int32_t gains_rows);

/* (still ABI 4: additions only -- look the symbols up to detect them) LEVELS of what a live handle or a tensor call emitted:
 * how loud the input, the background and the foreground of every slot were, whether anything repeating was found, whether a
 * stream clips or carries NaN -- reduced on the device, so that a server need not pull three signals to the host per hop. For
 * every stream s and channel c of an emission of n samples there are REPET_LEVEL_FIELDS float64 values, dense [S][C][8]: */
#define REPET_LEVEL_FIELDS 8
#define REPET_LEVEL_MIX_ENERGY 0   /* sum of mix^2 */
#define REPET_LEVEL_BG_ENERGY 1    /* sum of bg^2 */
#define REPET_LEVEL_FG_ENERGY 2    /* sum of fg^2 */
#define REPET_LEVEL_MIX_PEAK 3     /* max |mix| */
#define REPET_LEVEL_BG_PEAK 4      /* max |bg| */
#define REPET_LEVEL_FG_PEAK 5      /* max |fg| */
#define REPET_LEVEL_LIVE 6         /* number of live samples */
#define REPET_LEVEL_NONFINITE 7    /* number of live samples whose mixture is NaN or +-inf */
#define REPET_LEVEL_CHUNK 4096     /* samples of one stream a workgroup of the reduction takes */
/* mix, bg and fg are the float64 values the emission kernel forms for the sample BEFORE it rounds to the destination dtype, by
 * the same device function: mix = hi + lo (hi for an infinite hi), bg the fp32 background widened, fg = mix - bg or
 * fma(-a, bg, mix) with the gain that was in force for THAT emission, its fade included. The record therefore depends neither on
 * the output the handle has selected nor on a destination dtype. A sample that is not live -- every sample of an idle slot, the
 * samples before a slot's own first frame -- adds zero to every field and is not counted in LIVE, whatever the chunk carried
 * there. While a stream warms up BG_ENERGY is 0 and the FG fields equal the MIX fields. Energies are plain IEEE sums (NaN and
 * inf propagate); peaks skip NaN (fmax), are inf for an infinite sample and 0 with nothing live.
 * DETERMINISTIC: no floating-point atomics. The reduction has one fixed shape -- a thread's accumulators in element order, a wave
 * by __shfl_xor, the waves of a workgroup through LDS in wave order, the REPET_LEVEL_CHUNK-sample chunks of a long emission
 * through a partials buffer folded in a fixed order by a second small launch -- so two calls on one emission, the host form and
 * the device form, return identical bits. One launch for an emission of one chunk, two otherwise, a memset for an empty one
 * (a push that emitted nothing: all zeros). Computed ON DEMAND: a push that nobody asks about enqueues what it always did.
 * repet_online_last_levels        : host form, out[S][C][8] through the pinned buffer (one copy, one wait). out == NULL (or a
 *                   capacity too small) only asks: REPET_ERR_BAD_ARG with *n_written = the doubles needed.
 * repet_online_last_levels_device : dense float64 [S][C][8] at `dst` on the handle's device, ordered behind `signal_stream` by
 *                   events as last_emission_device is; no host wait.
 * Both are valid where last_emission is: after a push or finish, until the next push, finish, restart, release or import
 * (REPET_ERR_BAD_ARG, the same message); REPET_ERR_LIMIT where the emitted range is no longer in the pending buffer. S is the
 * handle's stream count. finish_stream drops its slot's samples, so it measures its tail itself ([C][8], S = 1: one launch more
 * in that call) -- but only on a handle that has been asked for levels before (any earlier call of either form, the asking one
 * included); on any other handle a finish_stream enqueues what it always did and the levels calls refuse as stale after it.
 * repet_ctx_result_levels_device  : the same record of the resident result of an offline context, [n_clips][C][8]: every
 *                   sample is live, the gain is the context's (repet_ctx_set_background_gain). Ordered as
 *                   repet_ctx_download_device_strided is (it waits for the remainder plane of a float64 upload where that does);
 *                   REPET_ERR_BAD_ARG for a context with no clip. More than 1024 channels: REPET_ERR_LIMIT (all three). */
int repet_online_last_levels(repet_online* h, double* out, int64_t capacity_doubles, int64_t* n_written);
int repet_online_last_levels_device(repet_online* h, void* dst, void* signal_stream);

/* (still ABI 4: additions only -- look the symbols up to detect them) The SPECTRA of the frames the last push completed, whole
 * or in bands: what a push decides is a time-frequency decision, and for every new frame of every slot the handle still holds
 * the mixture magnitudes and the masked spectrum until the next push writes there. For a frame j of a stream, channel c and bin
 * f in [0, F), F = window_length / 2 + 1, these are the reference's own quantities (repet.py:834-898), in fp32:
 *   REPET_OUT_MIXTURE     |audio_stft[f, j]|, as the forward kernel stored it, bit for bit
 *   REPET_OUT_BACKGROUND  mask[f] * mixture: the magnitude of the masked spectrum, by the device function the forward kernel
 *                         forms the mixture with -- so background == mixture to the bit wherever the mask is 1 (the high-pass
 *                         bins 1 .. cutoff_bins)
 *   REPET_OUT_FOREGROUND  mixture - background, and 0 where a rounding makes that negative; NaN where either is NaN
 * The frames covered are the n_frames the last push / finish completed: handle frames [first, first + n_frames), frame k
 * beginning at the caller's pushed sample k * step_length (first is counted in the caller's pushes, also on a handle whose
 * epoch an import of an older stream has moved). Per slot: a frame before the slot's own first frame -- the frame that straddles
 * a restart, every frame of an idle or held slot -- is ZERO in all three signals, whatever the chunk carried, NaN included; a
 * warm-up frame (the slot's own frame < start_frames - 1) has the mixture as it is, background 0 and foreground == mixture, as
 * in the time domain; finish's zero-padded last frame is a frame like any other.
 * Computed ON DEMAND from a small host record of the push: a push that nobody asks about enqueues what it always did. The record
 * is valid after a push or finish and STALE after the next push, finish, finish_stream, restart, release, import, hold or resume
 * (REPET_ERR_BAD_ARG): the frames of a finish_stream tail are not served. A push that completed no frame has n_frames = 0, and
 * the calls below then write nothing and launch nothing.
 * repet_online_last_frame_range          : first and n_frames, from the host record: no device work.
 * repet_online_last_frames               : host form, `which` as dense fp32 out[S][n_frames][C][F] through the pinned buffer
 *                   (one launch, one copy, one wait). out == NULL (or a capacity too small) only asks: REPET_ERR_BAD_ARG with
 *                   *n_written = the floats needed.
 * repet_online_last_frames_device        : the same values at `dst` on the handle's device, element (s, j, c, f) at
 *                   dst_strides[0] * s + [1] * j + [2] * c + [3] * f floats (non-negative; the elements must not overlap),
 *                   ordered behind `signal_stream` by events as last_emission_device is; one launch, no host wait.
 * repet_online_last_band_energies        : the same values reduced to bands: edges[0 .. n_bands] ascending (equal neighbours: an
 *                   empty band, 0) with 0 <= edges[k] <= F and 1 <= n_bands <= REPET_MAX_BANDS; band k is the float64 sum of
 *                   (double)m * (double)m over bins [edges[k], edges[k + 1]) of the fp32 value m above. Dense float64
 *                   out[S][n_frames][C][n_bands]; out == NULL or a capacity too small only asks, as above.
 * repet_online_last_band_energies_device : the same at `dst` (dense float64) on the handle's device, ordered as above.
 *                   The edges travel in the kernel's arguments: no copy, no host wait. One launch, which reads the handle's
 *                   rows itself (the full frames need not be written first). DETERMINISTIC: a lane adds its own bins in bin
 *                   order, a wave folds by __shfl_xor, no floating-point atomics -- two calls on one push, the host and the
 *                   device form, return identical bits. NaN and inf propagate as plain IEEE sums.
 * Errors, before anything is enqueued and with nothing changed: REPET_ERR_BAD_ARG for an unknown `which`, edges that are null,
 * descending or outside [0, F], n_bands < 1, a null destination or overlapping strides in the device forms, or a stale record;
 * REPET_ERR_LIMIT for more than REPET_MAX_BANDS bands. */
#define REPET_MAX_BANDS 128
int repet_online_last_frame_range(repet_online* h, int64_t* first_frame, int64_t* n_frames);
int repet_online_last_frames(repet_online* h, int which, float* out, int64_t capacity_floats, int64_t* n_written);
int repet_online_last_frames_device(repet_online* h, int which, void* dst, const int64_t dst_strides[4], void* signal_stream);
int repet_online_last_band_energies(repet_online* h, int which, const int32_t* edges, int32_t n_bands,
                                    double* out, int64_t capacity_doubles, int64_t* n_written);
int repet_online_last_band_energies_device(repet_online* h, int which, const int32_t* edges, int32_t n_bands,
                                           void* dst, void* signal_stream);

/* (still ABI 4: additions only -- look the symbols up to detect them) The SPECTRA OF A TENSOR CALL: the same three signals, under
 * the same contract, for the frames of the clip(s) an offline context separates (repet_ctx_execute / _async), without a second
 * STFT and without a host wait. An offline pipeline forgets its spectra as it goes -- a variant that works through a batch clip
 * by clip reuses the workspaces for the next clip --, so the request is ARMED on the context before the run and served behind
 * every pass of it:
 * repet_ctx_request_frames : arm. `which` as above. edges == NULL (n_bands 0): fp32 frames at `dst` on the context's device,
 *                   element (b, j, c, f) at dst_strides[0] * b + [1] * j + [2] * c + [3] * f floats (non-negative; the elements
 *                   must not overlap), for clip b < n_clips, frame j < T, channel c, bin f < F. edges != NULL: the float64 band
 *                   energies of repet_online_last_band_energies, dense dst[n_clips][T][C][n_bands] (dst_strides is ignored),
 *                   with the same deterministic reduction. T = repet_result_frame_count(algo, params, n_samples) with n_samples
 *                   the resident clip length (of a ragged batch: the pitch). The context's stream goes behind what
 *                   `signal_stream` has enqueued so far (the destination's earlier users); `signal_stream` goes behind the
 *                   launch that writes the last clip when the run is enqueued. A second request replaces the first.
 * repet_ctx_clear_requests : drop an armed request. Host only.
 * An armed request serves exactly the NEXT repet_ctx_execute / _async (or ranged execute) and is then dropped, also when that
 * execute fails. That execute refuses, with REPET_ERR_BAD_ARG and before it enqueues anything: REPET_EXTENDED and the ranged
 * executes (the segments overlap and cross-fade: there is no single spectrogram), a context whose resident samples are a window
 * of a longer clip (repet_ctx_set_window), band edges beyond F of the run's window_length, overlapping destination elements.
 * The frame grid: REPET_ORIGINAL, REPET_ADAPTIVE, REPET_SIM have T = ceil(n / H) + 1 frames, frame j beginning at sample
 * j * H - W / 2 (the reference's centred STFT); REPET_SIMONLINE has the online count, frame j beginning at sample j * H, and its
 * warm-up frames -- j < start_frames - 1 under repet_ctx_set_online_start, else j < buffer_frames - 1 -- have background 0 and
 * foreground == mixture. Of a ragged batch, clip b's frames at or past its OWN frame count are zero in all three signals,
 * whatever the padding holds (it is not read). The background is the magnitude of the masked bin as the variant's inverse STFT
 * fetches it: a pipeline leaves the masked spectrum in place (form 0), as the spectrum and a mask plane (1), or as the spectrum,
 * the repeating-segment model and the period (2), and the launch forms |X|, |X * mask| or |X * soft_mask(|X|, model)| with the
 * inverse kernels' own roundings -- in every form equal to the mixture, to the bit, in the high-pass bins. The spectra are the
 * plain call's: the background gains (scalar or by band) do not change them. Windows of 8192 samples are served (form 0).
 * A run with nothing armed enqueues exactly what it always did; a served one adds ONE launch per pass -- one for a single clip
 * and for the batches that go through every stage together, one per clip otherwise (repet_ctx_last_clip_passes) -- and a timing
 * stage "result_frames" behind the inverse STFT's (the longest stage list -- sim's on rank codes with every kernel marked
 * (REPET_RANK_OVERLAP=0), segment records by a pass of their own and band gains set -- then holds 13 of REPET_MAX_STAGES entries).
 * repet_result_frame_count      : T for `algo` and n_samples >= 0; -1 for REPET_EXTENDED, an unknown algo or bad params. Host
 *                   arithmetic, no device.
 * repet_ctx_last_spectrum_form  : the form (0, 1, 2) the last pass of the last run left; REPET_ERR_BAD_ARG before the first run. */
int repet_ctx_request_frames(repet_ctx* ctx, int which, const int32_t* edges /* nullable */, int32_t n_bands, void* dst,
                             const int64_t dst_strides[4], void* signal_stream);
int repet_ctx_clear_requests(repet_ctx* ctx);
int64_t repet_result_frame_count(int algo, const repet_params* params, int64_t n_samples);
int repet_ctx_last_spectrum_form(repet_ctx* ctx, int32_t* form);

/* (still ABI 4: additions only -- look the symbols up to detect them) The SIMILAR FRAMES the last push matched: for every frame
 * a live handle decides which earlier frames of the stream's buffer it resembles, and the frame's mask is the median over exactly
 * those (repet.py:855-866: the similarity vector of the frame against the buffer, its peaks, the list). For the n_frames frames
 * the last push / finish completed (repet_online_last_frame_range) and every slot, with K = repet_online_match_capacity:
 *   count       int32 [S][n_frames]     the length of the frame's list (repet.py:861-866), the frame itself included when it
 *                                       is in its own list -- its similarity with itself is 1, so it is unless an exact copy of
 *                                       it lies within similarity_distance
 *   age         int32 [S][n_frames][K]  entry k < count: how many of the stream's OWN frames back the similar frame lies, 0 the
 *                                       frame itself, 1 the frame before; strictly ascending (the order is by age, not by
 *                                       similarity, and not the engine's own); -1 for k >= count
 *   similarity  fp32  [S][n_frames][K]  the cosine similarity of the pair (repet.py:855-858), exactly the fp32 entry of the
 *                                       handle's similarity band that the peak picking read; 0 for k >= count
 * Own frames: a frame that passed while the slot was held does not exist for the slot, an imported stream's ages go on from
 * the exporting handle's, and under start_frames a stream's frame j holds min(buffer_frames, j + 1) frames, so age <= j.
 * A row has NO LIST -- count 0, every age -1, every similarity 0, whatever the chunk carried, NaN included -- for an idle or
 * held slot, the frame that straddles a restart, every warm-up frame (the slot's own frame < start_frames - 1) and a frame
 * whose similarity vector is NaN (a NaN sample in the frame: the reference's list is empty too).
 * Computed ON DEMAND from the host record of the push and what its peak picking left on the device: a push that nobody asks
 * about enqueues what it always did. Valid where repet_online_last_frames is: after a push or finish, STALE after the next
 * push, finish, finish_stream, restart, release, import, hold or resume (REPET_ERR_BAD_ARG); the frames of a finish_stream tail
 * are not served. A push that completed no frame has n_frames = 0: nothing is written and nothing launched.
 * repet_online_match_capacity       : K = min(similarity_number, ceil(buffer_frames / (similarity_distance_frames + 1))), the
 *                   most entries a list can have (repet.py:1294-1340: peaks at least similarity_distance apart, the
 *                   similarity_number largest kept). From the handle's parameters: no device work.
 * repet_online_last_matches         : host form, the three arrays dense as above through the pinned buffer (one launch, one
 *                   copy, one wait); *n_rows = S * n_frames. All three outputs NULL only asks for *n_rows (REPET_OK); one of
 *                   them NULL or capacity_rows < S * n_frames is REPET_ERR_BAD_ARG with *n_rows set.
 * repet_online_last_matches_device  : the same three dense arrays on the handle's device, ordered behind `signal_stream` by
 *                   events as last_emission_device is; one launch, no host wait. A null destination is REPET_ERR_BAD_ARG.
 * DETERMINISTIC: an entry's place is the number of entries of its list with a smaller age, counted inside one wavefront; no
 * atomics. Two calls on one push, the host and the device form, return identical bits. Asking changes nothing else. */
int repet_online_match_capacity(repet_online* h, int32_t* capacity);
int repet_online_last_matches(repet_online* h, int32_t* count_out, int32_t* age_out, float* similarity_out, int64_t capacity_rows,
                              int64_t* n_rows);
int repet_online_last_matches_device(repet_online* h, void* count_dst, void* age_dst, void* similarity_dst, void* signal_stream);

/* (still ABI 4: additions only -- look the symbols up to detect them) A stream that SITS OUT PUSHES. Pushes stay (S, n, C) in and
 * (S, n_emit, C) out, but a slot may be HELD: for as long as it is, time does not pass for its stream (silence suppression, a
 * lost or late packet, a caller whose clock lags). With P = samples per slot pushed so far and H the hop:
 * hold_streams    : the named live slots are held from the handle's sample P on. While a slot is held its share of every
 *                   pushed chunk is ignored (NaN and infinities included), its share of every emitted signal (background,
 *                   foreground, mixture, both outputs of one call, every destination dtype) is zero, last_levels counts
 *                   nothing for it (LIVE = 0), and nothing it holds changes: its rows of the similarity buffer, its last masked
 *                   spectrum, its held samples and their remainders stay as they are while the other slots' slide.
 * resume_streams  : the named held slots go on from the handle's sample P as if the pushes in between had not been made.
 * The guarantee: per slot, the output pieces of the pushes during which the slot was not held, concatenated in order and
 * followed by its finish_stream / finish tail, equal repet.simonline of the concatenated input pieces of those same pushes,
 * bit for bit -- whatever the other slots do and whatever the held chunks carried. The output runs one hop behind the input,
 * so the hop that belongs to the last input before a hold comes out of the first push after the resume; nothing is emitted
 * twice or dropped. The slot's first frame moves along with the handle (a held push of k hops adds k), so the stream's own
 * frame numbers, its circular positions and what start_frames counts are what they were.
 * Rules: hold and resume only where P % H == 0 (REPET_ERR_BAD_ARG otherwise, nothing changes: restart_streams' rule). While at
 * least one slot is held, a push of n % H != 0 samples is refused with REPET_ERR_BAD_ARG before anything is enqueued, so the
 * handle stays on the hop grid for as long as a hold lasts. An idle slot cannot be held and a slot out of range is refused
 * (REPET_ERR_BAD_ARG, nothing changes); holding a held slot and resuming a slot that is not held do nothing. restart_streams,
 * release_streams, import_stream and finish_stream on a held slot do what they always do and end the hold; finish ends held
 * slots like the others, each with its own length. export_stream of a held slot returns the stream as it stands (header and
 * payload unchanged, version 1): imported anywhere it goes on bit for bit. hold and resume make last_emission / last_levels
 * stale, as restart does. A background gain set for a held slot counts as covered by the emitting calls made meanwhile, as
 * for an idle slot: the fade elapses unheard and the new gain is in force at the resume.
 * stream_held     : *held = 1 where `slot` is held, 0 otherwise; answered on the host with no device work.
 * hold / resume enqueue one small launch per 256 slots named, with no host wait. A handle with no slot held enqueues per push
 * what it always did; a push with held slots enqueues the same number of launches (another slide kernel, and the background
 * alone goes through the kernel that emits the other signals). */
int repet_online_hold_streams(repet_online* h, const int32_t* slots, int32_t n_slots);
int repet_online_resume_streams(repet_online* h, const int32_t* slots, int32_t n_slots);
int repet_online_stream_held(repet_online* h, int32_t slot, int32_t* held);

/* (ABI 4) Per-slot inboxes: the slots of a handle of open_streams fed at their own pace. A push is in lockstep -- one chunk
 * [S][n][C] with one n -- while packets arrive per stream in sizes that never match the hop, late, in bursts or not at all.
 * With the inboxes the handle does the re-blocking itself. With H the hop, P the samples per slot pushed so far:
 * enable_feed     : every slot gets a FIFO of capacity_samples (>= H) samples per channel in device memory, held as the pending
 *                   buffers hold samples (fp32, and the fp32 remainder of float64 sources): S * capacity * C * 8 bytes. Once
 *                   per handle, at any age with P % H == 0. A handle that never calls it allocates nothing and enqueues what
 *                   it always did.
 * feed            : appends to the inboxes of the n_slots named slots: row i of the host array [n_slots][n][C] (REPET_F32 /
 *                   REPET_F64 / REPET_I16) brings its first counts[i] samples (counts null: all n) to slot slots[i]. What lies
 *                   behind counts[i] in a row is never read, NaN included; non-finite samples are let through as in a push.
 *                   All or nothing: REPET_ERR_BAD_ARG before anything is enqueued or changed for a slot out of range or named
 *                   twice, an idle slot, a count outside [0, n], a slot whose queued + count would exceed the capacity, and a
 *                   handle without inboxes or finished. A slot the caller holds may be fed: its queue grows. One staging copy
 *                   and one launch per 256 slots named; the values that later reach the pending buffers are bit for bit what
 *                   a push of them would have written.
 * feed_device     : the same from device memory (any ingest dtype, element strides [3] of [n_slots][n][C]): ordered behind
 *                   wait_stream, and signal_stream is made to wait for the copy, so the caller may overwrite the packet. No
 *                   host wait.
 * queued          : slot >= 0: *queued = the samples in that slot's inbox; slot < 0: queued[S], every slot's. Host counters.
 * pad_feed        : feeds each named slot (null: every live slot) (-queued) % H zeros, so that its queue ends on the hop grid,
 *                   and writes the pad counts to pads[n_slots] (pads[S] where slots is null). After the ticks that drain the
 *                   queue, the slot's finish_stream tail without its last `pad` samples is the stream's true tail. Refusals
 *                   as feed's.
 * clear_feed      : empties the inboxes of the named slots (null: of all). Host counters alone.
 * tick            : a lockstep push of hops * H samples whose chunk the handle assembles: requires P % H == 0. The READY slots
 *                   are the live slots that the caller does not hold and whose inbox has at least hops * H samples. Nobody
 *                   ready: nothing is enqueued, *n_written = 0, consumed[] all 0, and the handle, its last emission and its
 *                   records stay as they were. Otherwise every live slot the caller does not hold and that is not ready is
 *                   STARVED -- held for this push by the mechanism of hold_streams, the table written only for slots whose
 *                   state differs from the tick before -- each ready slot's oldest hops * H samples leave its inbox for the
 *                   pending buffers (one launch per 256 slots in the place of the push's append), and the push runs as ever:
 *                   out, the selected output, also_emit, last_emission, last_levels, last_frames and last_matches are the
 *                   push's, and a starved slot reads everywhere as a held one (zeros, LIVE = 0). consumed (nullable, [S]):
 *                   1 for the slots that took part. All decisions come from host counters; nothing is read back.
 * tick_device     : the same into a device destination, as push_device.
 * The guarantee is hold_streams', with starved ticks in the place of held pushes: per slot, the output pieces of the ticks
 * that consumed it, in order, followed by its finish_stream / finish tail, equal repet.simonline of the samples it consumed,
 * bit for bit, whatever the other slots did and in whatever packets the samples arrived.
 * With the rest of the handle: restart_streams, release_streams and import_stream empty the inboxes of their slots;
 * finish_stream, finish and stream_emit_count are refused (REPET_ERR_BAD_ARG, the message names clear_feed and pad_feed) while a
 * slot they end has queued samples; a plain push is refused while any inbox holds samples and otherwise first resumes the
 * starved slots (one launch) and is the push it always was; stream_held reports the caller's holds only, and resume_streams of
 * a starved slot leaves it held on the device until a tick finds it ready; export_stream returns the stream as consumed (the
 * queue is not part of the state, version 1). */
int repet_online_enable_feed(repet_online* h, int64_t capacity_samples);
int repet_online_feed(repet_online* h, const int32_t* slots, const int64_t* counts, int32_t n_slots, const void* audio, int dtype,
                      int64_t n);
int repet_online_feed_device(repet_online* h, const int32_t* slots, const int64_t* counts, int32_t n_slots, const void* src, int dtype,
                             int64_t n, const int64_t src_strides[3], void* wait_stream, void* signal_stream);
int repet_online_queued(repet_online* h, int32_t slot, int64_t* queued);
int repet_online_pad_feed(repet_online* h, const int32_t* slots, int32_t n_slots, int64_t* pads);
int repet_online_clear_feed(repet_online* h, const int32_t* slots, int32_t n_slots);
int repet_online_tick(repet_online* h, int64_t hops, double* out, int64_t capacity, uint8_t* consumed, int64_t* n_written);
int repet_online_tick_device(repet_online* h, int64_t hops, void* dst, int dst_dtype, const int64_t dst_strides[3], void* signal_stream,
                             uint8_t* consumed, int64_t* n_written);
int repet_ctx_result_levels_device(repet_ctx* ctx, void* dst, void* signal_stream);

/* (ABI 4) Self-test of the host conversions a staged upload / download runs (float64 -> fp32 samples + fp32 remainders,
 * fp32 -> float64; non-temporal AVX-512 / AVX2 lines where the CPU has them) against scalar loops on n values with NaN,
 * infinities, denormals, PCM-exact runs and every misalignment. No GPU needed. Returns the number of values that differ
 * (0 = pass). */
int64_t repet_host_conversion_selftest(int64_t n, uint32_t seed);

#ifdef __cplusplus
}
#endif
#endif /* REPET_HIP_H */
