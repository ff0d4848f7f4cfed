// the streaming handle: repet_online_* (see engine.h for the map of the engine's files)
#include "engine.h"

using namespace repet;
using namespace repet_eng;


// =====================================================================================================
// Streaming online REPET-SIM: the reference's "online" variant needs the whole signal
// (repet.py:712-911); this handle accepts audio in arbitrary chunks and returns each hop of background as
// soon as its frame has been seen, with the same kernels as the offline path, so the concatenated output is
// bit-identical to repet.simonline of the whole signal. Device state: a sliding window of the last B-1
// frames (magnitudes, unit rows, the last masked spectrum for the overlap-add tail) plus the unconsumed
// samples; every push processes all newly complete frames in one batch of launches.
// A handle of S streams is a handle of S slots: the pushes and the counters are shared, but a slot's own stream may begin
// later than the handle's (repet_online_restart_streams), end earlier (repet_online_finish_stream) or be absent
// (repet_online_release_streams). All of that is one number per slot, the frame at which its stream began, which the peak
// picking, the mask and the row zeroing behind the STFT read on the device; the launch shapes are the handle's.
// A slot may also sit out pushes (repet_online_hold_streams): held, it reads as idle on the device while its share of the buffers
// stays where it is (launch_slide_held) and its first frame moves along with the handle on the host.
// Every emitting call (push, tick, finish, finish_stream) has one body, online_*_impl; its host and device entry points differ in
// the Sink they build; every read-back call (last_*, export, import) likewise, online_read_*_impl behind a Reader. The waits on the
// caller's streams are the context's (engine.h: wait_caller / signal_caller), the pinned round trips of the host forms
// online_download / online_upload.
// =====================================================================================================
struct repet_online {
    repet_ctx* ctx = nullptr;       // stream, tables, tile cache, scratch buffers
    repet_params p{};
    int S = 1;                      // slots pushed in lockstep: the counters below are the handle's, the data is per slot
    // Which stream lives in a slot, and since when: slot s's own stream began at handle frame start[s] (sample start[s] * H;
    // kSlotIdle: no stream). slot_start is the same on the device, read by the peak picking, the mask and the row zeroing
    // once slots_on (a restart, release or finish_stream was made; until then every slot's stream is the handle's and no
    // kernel is given the table). latest_start: the largest frame a restart named; n_idle: idle slots.
    std::vector<int64_t> start;
    DevBuf slot_start;
    bool slots_on = false;
    int64_t latest_start = 0, n_idle = 0;
    // Held slots (repet_online_hold_streams): time does not pass for them. start[s] stays the slot's TRUE first frame and moves
    // along with the handle -- a held push of k hops adds k, on the host alone -- while the device table reads kSlotHeld for the
    // length of the hold: every kernel that is given the table takes the slot for idle, the slide (launch_slide_held) leaves
    // its share of the buffers where it is, and the resume writes start[s] back. One table, and no launch for the bump.
    std::vector<unsigned char> held;
    int64_t n_held = 0;
    // Inboxes (repet_online_enable_feed): every slot owns a ring of feed_cap samples per channel in `ring` (the hi plane of every
    // slot, then the lo plane; slot s at s * ring_stride floats of either), filled by repet_online_feed* at the slot's own pace
    // and emptied one lockstep chunk at a time by repet_online_tick*, which is a push whose chunk the handle takes from the
    // rings itself. q_count[s] / q_read[s]: the queued samples and the sample position of the oldest, host mirrors of what the
    // launches enqueued so far: the handle's stream orders the ring's reads and writes, and no call reads anything back. A live
    // slot that a tick finds short is STARVED: held for that push by the mechanism above. `held` stays what the device table
    // says -- held by either -- while caller_held / starved say by whom, so the table changes only where their OR does.
    // feed_cap == 0 (no enable_feed): none of this exists and every call enqueues what it always did.
    DevBuf ring;
    int64_t feed_cap = 0, ring_stride = 0;
    std::vector<int64_t> q_count, q_read;
    std::vector<unsigned char> caller_held, starved;
    float* ring_hi() const { return ring.as<float>(); }
    float* ring_lo() const { return ring.as<float>() + (int64_t)S * ring_stride; }
    int C = 0, W = 0, H = 0, F = 0, FS = 0, B = 0, Hh = 0, LP = 0;
    // start_frames (repet_online_set_start_frames; B: the reference): a stream's frames M-1 .. B-2 are separated on its buffer as
    // far as it has filled (peaks.h: row_columns). The handle's, for every slot and restart; the launches are the same for any M.
    int M = 0;
    // per stream s, at the strides below: X / V [C planes of rows_cap + kPadRows rows][FS], Vn [rows_cap rows][FS], the
    // pending samples [pend_cap][C] (pend_lo: their fp32 remainders), and in the per-push workspaces band / idx / cnt / outf
    DevBuf X[2], V[2], Vn[2], pend[2], pend_lo[2], band, outf, out64, staging;
    void* host_in = nullptr; size_t host_in_cap = 0;      // pinned: a host chunk on its way in, the result on its way out
    void* host_out = nullptr; size_t host_out_cap = 0;
    int cur = 0, pcur = 0;
    // the pending buffers start with `pend_hist` samples of HISTORY (already transformed: the frames of the sliding window,
    // whose float64 spectra the second level of the peak picking may ask for) followed by the pend_count unconsumed ones;
    // pend_lo: the fp32 remainders of float64 pushes, sample for sample
    int64_t pend_hist = 0;
    int64_t rows_cap = 0;           // frame rows per channel plane of the windows (without the 8 pad rows)
    int64_t pend_cap = 0, pend_count = 0;   // samples per channel
    int64_t hist_valid = 0;         // valid history rows, right-aligned at row Hh
    int64_t frames_done = 0, total_in = 0, emitted = 0;
    // hops by which imports of streams older than the handle moved its epoch (online_shift_epoch): the counters above read as
    // if the handle had been opened `epoch` hops earlier, and total_in - epoch * H is what the caller pushed per slot
    int64_t epoch = 0;
    int64_t max_push = 0;           // repet_online_open_streams: windows and pending buffers sized for pushes of this many samples
    bool finished = false;
    // What the emitting calls deliver (repet_online_set_output), the one-shot second destination of the next one
    // (repet_online_also_emit), and where the samples of the last emission lie: the emitted range [pos0, pos0 + n) is the front
    // of the unconsumed samples of the pending buffer `buf` AS IT WAS BEFORE THE SLIDE (`off` samples into every stream's
    // share). Nothing writes that buffer before the next push's slide; restart / release and the next append end its validity.
    int out_which = REPET_OUT_BACKGROUND;
    struct Also { int which = -1; void* dst = nullptr; int dtype = REPET_F64; int64_t strides[3] = {0, 0, 0}; } also;
    // (g0, g1, ramp: the gain tables of that emission, see below -- a fade from table g0 to table g1 over its first `ramp` samples;
    // shaped: its foreground is formed from the shaped background in `outs`, see the band gains below)
    struct Emission { bool valid = false; int buf = 0, S = 0, slot = -1; int64_t off = 0, n = 0, pos0 = 0; int g0 = 0, g1 = 0; int64_t ramp = 0; bool shaped = false; } em;
    // Background gains (repet_online_set_background_gain): the foreground of slot s is x - a[s] * bg, a = (float)(1 - gain). The
    // gain is the SLOT's: no restart, release, finish_stream or import touches it. gain[s] is the host mirror of what was set;
    // gain_tab holds three fp32 tables [S] on the device, all 1 at open: the target (written by a set, entry for entry, with no
    // host wait) and two current tables, of which `gcur` is in force. A set marks its slots dirty; the first emitting call that
    // covers a dirty slot writes the OTHER current table (target where it covers, the table in force elsewhere: one small
    // launch), fades from the one to the other over min(H, n_emit) samples and puts the other in force. Both stay as they are
    // until the next fade, so last_emission replays a fade from the tables that made it, whatever was set since. Until the first
    // set (gains_on) no kernel is given a table.
    // Levels (repet_online_last_levels*): computed on demand from what `em` describes, so a handle that is never asked runs
    // nothing for them. `levels` holds the record of a finish_stream tail ([C][8] float64): that call drops its slot's samples, so
    // it measures the tail itself -- on a handle that has been asked for levels before (levels_on) -- and tail_valid says the kept
    // record is the last emission's.
    DevBuf levels;
    bool levels_on = false, tail_valid = false;
    double* tail_levels() const { return levels.as<double>(); }
    // Frames (repet_online_last_frames* / last_band_energies*): where the spectra of the frames the last push or finish completed
    // lie. After the push's slide flipped `cur` they are rows [row0, row0 + n) of every slot's planes of X[win] / V[win], the
    // window that was current DURING the push; the first of them is handle frame `first`. Nothing writes that window before
    // the next push. Host record only: a handle that is never asked runs nothing for it. Every call that changes the slot
    // table ends its validity with the emission's, so the table at query time is the table of the push.
    struct Frames { bool valid = false; int win = 0, S = 0; int64_t row0 = 0, n = 0, first = 0; } fr;
    // Matches (repet_online_last_matches*): where the similar-frame lists of those frames lie. The push left them in the context's
    // idx / cnt (list row r belongs to record frame n - n_active + r; idx_pitch entries per row, the slots n_active rows apart)
    // as rows of the window counted from its first valid row, where record frame 0 is row `hist`; the similarities the peak
    // picking read are still in `band` (band_stride floats per slot), in the look-back layout or the diagonal one. Nothing
    // between a push and the next call that ends the record's validity writes any of the three: the levels, frames, gain and
    // band-gain launches have buffers of their own, and finish_stream, which runs the peak picking again, ends the validity.
    // n_active == 0: the push picked no peaks (every frame a warm-up frame) and the buffers are not read.
    struct Matches { int64_t n_active = 0, hist = 0, band_stride = 0; int idx_pitch = 0; bool lookback = false; } mt;
    std::vector<float> gain;
    std::vector<unsigned char> gain_dirty;
    int64_t n_dirty = 0;
    DevBuf gain_tab;
    int gcur = 0;
    bool gains_on = false;
    float* gain_target() const { return gain_tab.as<float>(); }
    float* gain_current(int k) const { return gain_tab.as<float>() + (int64_t)(1 + k) * S; }
    // Band gains (repet_online_set_background_band_gains): the foreground of slot s takes a SHAPED background, the overlap-add
    // inverse of a[k] * Y_j[k] with a = (float)(1 - g) per bin, in place of the plain one. The inverse is linear and a frame is
    // shaped once and whole, with the table its slot had when the call that completed it was enqueued; a frame rings into two
    // hops, so the frame carried over from the call before needs the table IT was completed under. band_tab holds three rows of
    // FS factors per slot (engine.h: bands): carried, new, pending. A set writes the pending row (one launch, the gains read from a
    // pinned job buffer: no copy, no wait) and marks the slot; every call that inverts first brings the rows of its slots up to
    // date where a mark says so (one launch: carried = new, and where it completes frames new = pending), which is twice after
    // a set -- the second time for the carried row alone -- and never again. Held slots keep rows and marks until they resume.
    // band_stale[s]: bit 0 new != pending, bit 1 carried != new. band_nd[s]: bits 0 / 1 / 2 the pending / new / carried row is not
    // all ones. While any slot has a bit of band_nd the emitting calls run the inverse a second time, with the rows, into `outs`
    // beside outf, and em.shaped says that the foreground of that emission reads it. The tables belong to the slots (no
    // restart, release, finish_stream or import touches them; an import settles its slot: all three rows = pending) and exist
    // from the first set on (bands_on): until then nothing here costs a launch.
    DevBuf band_tab, outs;
    bool bands_on = false;
    std::vector<std::vector<float>> band_gain;          // g as last set, per slot (empty: all zero)
    std::vector<unsigned char> band_stale, band_nd;
    int64_t n_band_stale = 0, n_band_nd = 0;            // slots with a bit of either
    static constexpr int kBandJobs = 4;
    struct BandJob { void* p = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool busy = false; } band_job[kBandJobs];
    int band_job_next = 0;
    float* band_rows(int64_t slot) const { return band_tab.as<float>() + slot * kBandRows * FS; }
    void band_mark(size_t s, unsigned char stale, unsigned char nd) {
        n_band_stale += (stale != 0) - (band_stale[s] != 0);
        n_band_nd += (nd != 0) - (band_nd[s] != 0);
        band_stale[s] = stale; band_nd[s] = nd;
    }

    int64_t plane() const { return (rows_cap + kPadRows) * FS; }        // elements between channel planes of X and V
    int64_t spec_stride() const { return (int64_t)C * plane(); }      // ... between streams in X and V
    int64_t vn_stride() const { return rows_cap * FS; }               // ... between streams in Vn
    int64_t pend_stride() const { return pend_cap * C; }              // ... between streams in pend / pend_lo
};

namespace repet_eng {

static void free_pinned(void*& p, size_t& cap) {
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
}

static int ensure_pinned(void*& p, size_t& cap, size_t bytes) {
    if (bytes <= cap) return REPET_OK;
    free_pinned(p, cap);
    const size_t want = std::max<size_t>((bytes + 4095) & ~size_t(4095), 4096);
    HIP_TRY(hipHostMalloc(&p, want, hipHostMallocDefault));
    cap = want;
    return REPET_OK;
}

// The pinned round trips of the host forms, once each. Down: `bytes` of device memory into the pinned buffer, one copy and one
// wait; the caller copies on from o->host_out (several scatter one block into two or three arrays).
static int online_download(repet_online* o, const void* dev, size_t bytes) {
    repet_ctx* c = o->ctx;
    RP_TRY(ensure_pinned(o->host_out, o->host_out_cap, bytes));
    HIP_TRY(hipMemcpyAsync(o->host_out, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return REPET_OK;
}

// Up: `bytes` of the caller's memory through the pinned buffer on their way into o->staging.
static int online_upload(repet_online* o, const void* host, size_t bytes) {
    repet_ctx* c = o->ctx;
    HIP_TRY(hipStreamSynchronize(c->stream));          // a device call may still be running; the pinned buffer is free
    RP_TRY(ensure_pinned(o->host_in, o->host_in_cap, bytes));
    HIP_TRY(o->staging.ensure(bytes));
    std::memcpy(o->host_in, host, bytes);
    HIP_TRY(hipMemcpyAsync(o->staging.p, o->host_in, bytes, hipMemcpyHostToDevice, c->stream));
    return REPET_OK;
}

// The records of the last emitting call (its emission, a finish_stream tail's levels, its frames and with them its matches) end
// with every call that appends samples (push, tick) or changes the slot table (restart, release, finish_stream, import, hold,
// resume): what the records point at is about to be overwritten, or the table at query time would not be the call's.
static void online_invalidate_records(repet_online* o) {
    o->em.valid = false; o->tail_valid = false; o->fr.valid = false;
}

static int check_slot(const repet_online* o, int32_t slot) {
    if (slot < 0 || slot >= o->S) return fail(REPET_ERR_BAD_ARG, "online: slot out of range");
    return REPET_OK;
}

int online_ensure_windows(repet_online* o, int64_t n_new) {
    repet_ctx* c = o->ctx;
    const int64_t need = round_up(o->Hh + n_new, kTile) + kTile;
    if (need <= o->rows_cap) return REPET_OK;
    const int64_t new_cap = std::max(need, 2 * o->rows_cap);
    HIP_TRY(hipStreamSynchronize(c->stream));
    DevBuf nx, nv, nvn;
    const size_t plane = (size_t)(new_cap + kPadRows) * o->FS;
    const size_t planes = plane * o->C * o->S;
    const size_t vn = (size_t)new_cap * o->FS * o->S;
    HIP_TRY(nx.ensure(planes * sizeof(float2)));
    HIP_TRY(nv.ensure(planes * sizeof(float)));
    HIP_TRY(nvn.ensure(vn * sizeof(float)));
    HIP_TRY(hipMemsetAsync(nx.p, 0, planes * sizeof(float2), c->stream));
    HIP_TRY(hipMemsetAsync(nv.p, 0, planes * sizeof(float), c->stream));
    HIP_TRY(hipMemsetAsync(nvn.p, 0, vn * sizeof(float), c->stream));
    if (o->hist_valid > 0) {        // carry the history (rows [Hh - hist_valid, Hh)) of every stream into the bigger window
        const int64_t r0 = o->Hh - o->hist_valid, len = o->hist_valid * o->FS;
        const int64_t op = o->plane(), np = (int64_t)plane;
        const RowCopy parts[3] = {
            {o->Vn[o->cur].as<float>() + r0 * o->FS, nvn.as<float>() + r0 * o->FS, len, 1, 0, 0, o->vn_stride(), new_cap * o->FS},
            {o->V[o->cur].as<float>() + r0 * o->FS, nv.as<float>() + r0 * o->FS, len, o->C, op, np, o->C * op, o->C * np},
            {o->X[o->cur].as<float>() + 2 * r0 * o->FS, nx.as<float>() + 2 * r0 * o->FS, 2 * len, o->C, 2 * op, 2 * np, 2 * o->C * op, 2 * o->C * np}};
        HIP_TRY(launch_row_copies(parts, 3, o->S, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    o->X[o->cur].release(); o->V[o->cur].release(); o->Vn[o->cur].release();
    o->X[o->cur] = nx; o->V[o->cur] = nv; o->Vn[o->cur] = nvn;
    // the other window is only ever written after being (re)initialised below
    o->X[o->cur ^ 1].release(); o->V[o->cur ^ 1].release(); o->Vn[o->cur ^ 1].release();
    HIP_TRY(o->X[o->cur ^ 1].ensure(planes * sizeof(float2)));
    HIP_TRY(o->V[o->cur ^ 1].ensure(planes * sizeof(float)));
    HIP_TRY(o->Vn[o->cur ^ 1].ensure(vn * sizeof(float)));
    HIP_TRY(hipMemsetAsync(o->X[o->cur ^ 1].p, 0, planes * sizeof(float2), c->stream));
    HIP_TRY(hipMemsetAsync(o->V[o->cur ^ 1].p, 0, planes * sizeof(float), c->stream));
    HIP_TRY(hipMemsetAsync(o->Vn[o->cur ^ 1].p, 0, vn * sizeof(float), c->stream));
    o->rows_cap = new_cap;
    // the streams' channel planes follow each other at the same stride: S x C planes for the pad rows
    for (int k = 0; k < 2; ++k)
        HIP_TRY(launch_fill_pad_rows(o->V[k].as<float>(), (new_cap + kPadRows) * o->FS, o->C * o->S, new_cap, o->FS, c->stream));
    return REPET_OK;
}

// room for `n` more samples per stream in the pending buffers (a multiple of 4 samples: 16-byte aligned streams)
int online_ensure_pending(repet_online* o, int64_t n) {
    repet_ctx* c = o->ctx;
    const int64_t need = o->pend_hist + o->pend_count + n;
    if (need <= o->pend_cap) return REPET_OK;
    const int64_t cap = round_up(std::max<int64_t>(need + o->W + (int64_t)o->Hh * o->H, 2 * o->pend_cap), 4);
    const size_t bytes = (size_t)cap * o->C * o->S * sizeof(float);
    DevBuf a, b, al, bl;
    HIP_TRY(a.ensure(bytes));
    HIP_TRY(b.ensure(bytes));
    HIP_TRY(al.ensure(bytes));
    HIP_TRY(bl.ensure(bytes));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int64_t live = (o->pend_hist + o->pend_count) * o->C;
    if (live > 0) {
        const RowCopy parts[2] = {{o->pend[o->pcur].as<float>(), a.as<float>(), live, 1, 0, 0, o->pend_stride(), cap * o->C},
                                  {o->pend_lo[o->pcur].as<float>(), al.as<float>(), live, 1, 0, 0, o->pend_stride(), cap * o->C}};
        HIP_TRY(launch_row_copies(parts, 2, o->S, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    o->pend[0].release(); o->pend[1].release(); o->pend_lo[0].release(); o->pend_lo[1].release();
    o->pend[0] = a; o->pend[1] = b; o->pend_lo[0] = al; o->pend_lo[1] = bl; o->pcur = 0; o->pend_cap = cap;
    return REPET_OK;
}

// Process n_new frames of every stream starting at global frame o->frames_done (the samples are at the front of the pending
// buffers; samples past pend_count read as zero) and leave `n_emit` output samples per stream and channel, starting at the
// first sample of hop frames_done, in outf [S][n_emit][C] (fp32). Enqueues only: no host wait unless a buffer grows. One
// fixed sequence of launches, whatever S and C.
// slot >= 0 (finish_stream): the same sequence on that slot alone (a batch of one at the slot's offsets), with no slide and
// no counter touched: the handle goes on as if the call had not been made.
// n_app: the samples per stream this push appended. While slots are held the slide has to know: their share of the pending
// buffers ends n_app samples before the others' does, and their first frames move on by n_app / H.
int online_process(repet_online* o, int64_t n_new, int64_t n_emit, int slot = -1, int64_t n_app = 0) {
    repet_ctx* c = o->ctx;
    o->em = repet_online::Emission{true, o->pcur, slot < 0 ? o->S : 1, slot, o->pend_hist, std::max<int64_t>(n_emit, 0), o->emitted};
    o->tail_valid = false;
    o->em.g0 = o->em.g1 = o->gcur;
    // (the new frames' rows follow the history in the current window; a finish_stream tail's frames are not served)
    o->fr = repet_online::Frames{slot < 0, o->cur, o->S, o->Hh, std::max<int64_t>(n_new, 0), o->frames_done};
    o->mt = repet_online::Matches{};
    // (a held push that completes no frame -- a handle younger than a window -- still slides the samples: the held slots' stay)
    const bool held_push = slot < 0 && o->n_held > 0 && n_app > 0;
    if (n_new <= 0 && n_emit <= 0 && !held_push) return REPET_OK;
    Tables* tb = nullptr;
    RP_TRY(get_tables(c, o->W, &tb));
    RP_TRY(online_ensure_windows(o, n_new));
    const bool all = slot < 0;
    const int S = all ? o->S : 1;
    const int64_t sb = all ? 0 : slot;
    const int64_t plane = o->plane();                            // chan_stride of X and V
    const int64_t spec = o->spec_stride(), vns = o->vn_stride(), pst = o->pend_stride();
    const int64_t r0 = o->Hh - o->hist_valid;                    // first valid window row
    const int64_t Tw = o->hist_valid + n_new;                    // valid rows (history + new), relative to r0
    float2* Xb = o->X[o->cur].as<float2>() + sb * spec + r0 * o->FS;
    float* Vb = o->V[o->cur].as<float>() + sb * spec + r0 * o->FS;
    float* Vnb = o->Vn[o->cur].as<float>() + sb * vns + r0 * o->FS;
    const float* pend = o->pend[o->pcur].as<float>() + sb * pst;
    const float* pend_lo = o->pend_lo[o->pcur].as<float>() + sb * pst;
    const int64_t first_global = o->frames_done - o->hist_valid; // global frame number of window row r0
    const int64_t* starts = o->slots_on ? o->slot_start.as<int64_t>() + sb : nullptr;      // the slots' own first frames
    // REPET_FLAG_SILENT_FRAMES_ZERO: the forward kernel flags the silent frames among the n_new of this push (one word each, slot
    // after slot) beside their unit rows; the peak picking reads silence off the band, the mask kernels off the table. Nothing
    // of it outlives the push: no slide, no readback, no launch more. A handle without the bit hands out no table.
    const bool silent_zero = (o->p.flags & REPET_FLAG_SILENT_FRAMES_ZERO) != 0;
    SilentZeroScope silent_scope(c, silent_zero);

    if (n_new > 0) {
        StftArgs a{};
        a.audio = pend; a.n_samples = o->pend_count; a.n_channels = o->C; a.sample_offset = o->pend_hist;
        a.window = tb->window.as<float>(); a.twiddle = tb->twiddle.as<float2>();
        a.W = o->W; a.H = o->H; a.T = n_new; a.FS = o->FS; a.centred = 0;
        a.X = Xb + o->hist_valid * o->FS; a.V = Vb + o->hist_valid * o->FS; a.chan_stride = plane;
        a.Vn = Vnb + o->hist_valid * o->FS;
        a.n_batch = S; a.batch_sample_stride = o->pend_cap; a.batch_spec_stride = spec; a.batch_mean_stride = vns;
        if (silent_zero) {
            HIP_TRY(c->silent.ensure((size_t)S * n_new * sizeof(unsigned int)));
            a.silent = c->silent.as<unsigned int>(); a.batch_silent_stride = n_new;
        }
        HIP_TRY(launch_stft(a, c->stream));
        // rows behind the new frames up to the next tile boundary must read as zero for the Gram tiles
        const int64_t Tpad = round_up(Tw, kTile);
        // (same launch) the new rows of frames before a slot's own first frame -- the frame that straddles a restart, every
        // frame of an idle slot -- hold nothing of that slot's stream: zero in Vn, V and X, whatever the chunk carried
        const bool early = starts && (o->n_idle > 0 || o->n_held > 0 || o->latest_start > o->frames_done);
        const int64_t hv = o->hist_valid * o->FS, nn = n_new * o->FS;
        const RowCopy zero[4] = {
            {nullptr, Vnb + Tw * o->FS, (Tpad - Tw) * o->FS, 1, 0, 0, 0, vns},
            {nullptr, Vnb + hv, nn, 1, 0, 0, 0, vns, o->FS, o->frames_done},
            {nullptr, Vb + hv, nn, o->C, 0, plane, 0, spec, o->FS, o->frames_done},
            {nullptr, reinterpret_cast<float*>(Xb) + 2 * hv, 2 * nn, o->C, 0, 2 * plane, 0, 2 * spec, 2 * (int64_t)o->FS, o->frames_done}};
        HIP_TRY(launch_row_copies(zero, early ? 4 : 1, S, c->stream, starts));

        const int64_t first_active = std::max<int64_t>(o->frames_done, o->M - 1);     // global frame number
        const int64_t n_active = o->frames_done + n_new - first_active;
        const int K = o->p.sim_number, KP = std::max(K, kMinIdxPitch);
        if (n_active > 0) {
            const int64_t band_stride = Tpad * o->LP;
            HIP_TRY(o->band.ensure((size_t)S * band_stride * sizeof(float)));
            RP_TRY(run_gram_band(c, Vnb, Tw, o->FS, o->band.as<float>(), o->B, o->LP, true, S, vns, band_stride, false, true));
            const int peak_mode = c->band_lookback ? 2 : 1;
            HIP_TRY(c->idx.ensure((size_t)S * n_active * KP * sizeof(int32_t)));
            HIP_TRY(c->cnt.ensure((size_t)S * n_active * sizeof(int32_t)));
            PeakRefine rf{};
            RP_TRY(make_refine(c, Vnb, o->FS, o->p.sim_threshold, &rf, n_active, S, o->B, o->p.sim_distance_frames, Tpad));
            const PeakBatch pb{S, band_stride, n_active * KP, n_active, vns, starts, o->M};
            const PeakBatch* batch = (S > 1 || starts) ? &pb : nullptr;
            hipError_t e = launch_local_maxima(o->band.as<float>(), n_active, first_active, o->B, o->LP, peak_mode, (float)o->p.sim_threshold,
                                               o->p.sim_distance_frames, K, c->idx.as<int32_t>(), KP, c->cnt.as<int32_t>(), c->stream,
                                               first_global, &rf, batch);
            if (e == hipErrorInvalidValue) return fail(REPET_ERR_LIMIT, "online: buffer too long for the peak-picking kernel");
            HIP_TRY(e);
            // second level: window row fr is global frame first_global + fr, whose first sample sits hist_valid - fr hops
            // before the pending ones in ITS stream's buffer (zero beyond what has been pushed, as in the offline run's last frame)
            const Geo go = make_geo(o->W, o->H, Tw, o->C);
            RP_TRY(run_exact_rows(c, tb, go, o->band.as<float>(), first_active, o->B, o->LP, peak_mode, (float)o->p.sim_threshold,
                                  o->p.sim_distance_frames, K, c->idx.as<int32_t>(), KP, c->cnt.as<int32_t>(), first_global, rf,
                                  batch, pend, pend_lo,
                                  o->pend_hist + o->pend_count, pst, o->pend_hist - o->hist_valid * (int64_t)o->H, Tpad, S));
            o->mt = repet_online::Matches{n_active, o->hist_valid, band_stride, KP, c->band_lookback};
        }
        MaskArgs m{};
        m.V = Vb; m.chan_stride = plane; m.n_channels = o->C; m.T = Tw; m.F = o->F; m.FS = o->FS; m.X = Xb; m.mask = nullptr;
        m.cutoff = o->p.cutoff_bins; m.pad_row = o->rows_cap - r0; m.frame0 = o->hist_valid;
        m.n_batch = S; m.batch_stride = spec;
        m.slot_start = starts; m.slot_bias = first_global - (o->M - 1);     // row t is the slot's frame first_global + t - start
        if (silent_zero) { m.silent = c->silent.as<unsigned int>(); m.silent_batch_stride = n_new; }      // (row frame0 + k: new frame k)
        m.idx_batch_stride = std::max<int64_t>(n_active, 0) * KP; m.cnt_batch_stride = std::max<int64_t>(n_active, 0);
        const int64_t first_frame = Tw - std::max<int64_t>(n_active, 0);          // warm-up rows before it are zeroed
        const int max_peaks = (int)std::min<int64_t>(K, ceil_div(o->B, o->p.sim_distance_frames + 1));
        HIP_TRY(launch_mask_sim(m, c->idx.as<int32_t>(), KP, c->cnt.as<int32_t>(), first_frame, max_peaks, c->stream));
    }
    if (n_emit > 0) {
        HIP_TRY(o->outf.ensure((size_t)S * n_emit * o->C * sizeof(float)));
        IstftOlaArgs a{};
        a.Y = Xb; a.chan_stride = plane; a.n_channels = o->C; a.T = Tw; a.FS = o->FS; a.W = o->W;
        a.twiddle = tb->twiddle.as<float2>(); a.trim = o->hist_valid * (int64_t)o->H; a.out = o->outf.as<float>();
        a.n_out = n_emit; a.out_offset = 0; a.scale = (float)(1.0 / tb->cola);
        a.n_batch = S; a.batch_first = 0; a.batch_step = 1; a.batch_total = S; a.batch_local0 = 0;
        a.batch_spec_stride = spec; a.batch_out_stride = n_emit; a.overlap = 0;
        RP_TRY(istft_rc(launch_istft_ola(a, c->stream)));
        if (o->bands_on) {
            // band gains: the rows of the slots this call inverts, brought up to date where a set (or the call before) left a mark
            const int mode = n_new > 0 ? kBandCommit : kBandCarry;
            const unsigned char due = n_new > 0 ? 3 : 2;
            auto step = [&](size_t s) {
                const unsigned char st = o->band_stale[s], nd = o->band_nd[s];
                const unsigned char carried = (nd & 2) ? 4 : 0;                      // carried = new
                if (n_new > 0) o->band_mark(s, (st & 1) ? 2 : 0, (unsigned char)((nd & 1) | ((nd & 1) ? 2 : 0) | carried));
                else o->band_mark(s, st & 1, (unsigned char)((nd & 3) | carried));
            };
            if (all && o->n_band_stale > 0) {
                bool any = false;
                for (size_t s = 0; s < (size_t)o->S; ++s)
                    if (!o->held[s] && (o->band_stale[s] & due)) { any = true; step(s); }
                if (any) HIP_TRY(launch_band_commit(o->band_tab.as<float>(), o->FS, o->S, -1, mode, o->slots_on ? o->slot_start.as<int64_t>() : nullptr, c->stream));
            } else if (!all && (o->band_stale[(size_t)slot] & due)) {
                step((size_t)slot);
                HIP_TRY(launch_band_commit(o->band_tab.as<float>(), o->FS, o->S, slot, mode, nullptr, c->stream));
            }
        }
        if (o->n_band_nd > 0) {
            // some slot's rows are not all ones: the same inverse once more, every bin times its slot's factor as it is fetched,
            // into the buffer the foreground of this emission reads (a slot whose rows are all ones gets the plain bits)
            HIP_TRY(o->outs.ensure((size_t)S * n_emit * o->C * sizeof(float)));
            a.out = o->outs.as<float>();
            a.G = o->band_rows(sb); a.G_batch_stride = (int64_t)kBandRows * o->FS; a.G_split = o->hist_valid;
            RP_TRY(istft_rc(launch_istft_ola(a, c->stream)));
            o->em.shaped = true;
        }
    }
    if (n_emit > 0 && o->gains_on && (all ? o->n_dirty > 0 : o->gain_dirty[(size_t)slot] != 0)) {
        // a gain was set since these slots last emitted: this emission fades to it, and it is in force afterwards
        // (the min below is a guard only: online_plan emits whole hops from a push and H + ((N - W) mod H) samples, or all N >=
        // H of a short stream, from a finish, so n_emit >= H wherever n_emit > 0 and no emission is shorter than a fade)
        const int nxt = o->gcur ^ 1;
        HIP_TRY(launch_gain_commit(o->gain_target(), o->gain_current(o->gcur), o->gain_current(nxt), o->S, all ? -1 : slot, c->stream));
        o->em.g0 = o->gcur; o->em.g1 = nxt; o->em.ramp = std::min<int64_t>(o->H, n_emit);
        o->gcur = nxt;
        if (all) { std::fill(o->gain_dirty.begin(), o->gain_dirty.end(), 0); o->n_dirty = 0; }
        else { o->gain_dirty[(size_t)slot] = 0; o->n_dirty -= 1; }
    }
    if ((n_new > 0 || held_push) && all) {
        // slide, one launch for every stream and channel: the last min(Hh, Tw) rows of V and Vn and the last masked spectrum
        // (overlap-add tail of the next hop) become the history of the other window; the samples of the window's frames
        // (h2 hops of history) and the unconsumed ones move to the front of the other pending buffer
        const int64_t h2 = std::min<int64_t>(o->Hh, Tw);
        const int nxt = o->cur ^ 1;
        const int64_t src = r0 + Tw - h2, dst = o->Hh - h2;
        const int64_t consumed = std::min<int64_t>(n_new * (int64_t)o->H, o->pend_count);
        const int64_t left = o->pend_count - consumed;
        const int64_t keep = std::min<int64_t>(h2 * (int64_t)o->H, o->pend_hist + consumed);
        const int64_t from = o->pend_hist + consumed - keep;
        const int64_t FS = o->FS;
        const int64_t rows = n_new > 0 ? 1 : 0;                 // (no new frame: the windows stay, only the samples move)
        const RowCopy parts[kRowCopyParts] = {
            {o->Vn[o->cur].as<float>() + src * FS, o->Vn[nxt].as<float>() + dst * FS, rows * h2 * FS, 1, 0, 0, vns, vns},
            {o->V[o->cur].as<float>() + src * FS, o->V[nxt].as<float>() + dst * FS, rows * h2 * FS, o->C, plane, plane, spec, spec},
            {o->X[o->cur].as<float>() + 2 * (r0 + Tw - 1) * FS, o->X[nxt].as<float>() + 2 * (o->Hh - 1) * FS, rows * 2 * FS, o->C,
             2 * plane, 2 * plane, 2 * spec, 2 * spec},
            {o->pend[o->pcur].as<float>() + from * o->C, o->pend[o->pcur ^ 1].as<float>(), (keep + left) * o->C, 1, 0, 0, pst, pst},
            {o->pend_lo[o->pcur].as<float>() + from * o->C, o->pend_lo[o->pcur ^ 1].as<float>(), (keep + left) * o->C, 1, 0, 0, pst, pst}};
        if (o->n_held > 0) {
            // A held slot's share stays as it is, right-aligned like everybody's: its history rows [Hh - hist_valid, Hh) of the
            // current window become the same rows of the other one, the h2 - hist_valid rows in front of them (a history that
            // still grows) zero; its held samples [0, pend_hist + pend_count - n_app) -- what it held before this push's chunk
            // was appended behind them -- end where the others' end, behind `shift` zeros. Relative to the parts' sources:
            //   rows     (src - dst) = n_new rows back: reads rows [Hh - hist_valid, Hh) of the current window
            //   spectrum row r0 + Tw - 1 -> row Hh - 1, n_new rows back (nothing to keep while the handle has no history)
            //   samples  from + shift = n_app samples back: reads [0, pend_hist + pend_count - n_app) of the stream's share
            // and never in front of a share: below zero_below the source is not read.
            const int64_t grow = h2 - o->hist_valid, before = o->pend_count - n_app;
            const int64_t shift = keep + left - o->pend_hist - before;
            if (grow < 0 || before < 0 || shift < 0 || from + shift != n_app)
                return fail(REPET_ERR_LIMIT, "online: a held stream does not fit the slide");
            const HeldShift shifts[kRowCopyParts] = {{-n_new * FS, grow * FS}, {-n_new * FS, grow * FS},
                                                     {-2 * n_new * FS, o->hist_valid > 0 ? 0 : 2 * FS},
                                                     {-n_app * o->C, shift * o->C}, {-n_app * o->C, shift * o->C}};
            HIP_TRY(launch_slide_held(parts, shifts, kRowCopyParts, S, c->stream, o->slot_start.as<int64_t>()));
        } else {
            HIP_TRY(launch_row_copies(parts, kRowCopyParts, S, c->stream));
        }
        if (n_new > 0) {
            o->cur = nxt;
            o->hist_valid = h2;
            o->frames_done += n_new;
        }
        o->pcur ^= 1;
        o->pend_hist = keep;
        o->pend_count = left;
        if (held_push) {
            // time did not pass for the held slots: their first frames move on with the handle
            const int64_t hops = n_app / o->H;
            for (size_t s = 0; s < o->held.size(); ++s)
                if (o->held[s]) { o->start[s] += hops; o->latest_start = std::max(o->latest_start, o->start[s]); }
        }
    }
    if (all) o->emitted += n_emit;
    return REPET_OK;
}

// what a push of n samples per stream (finishing = false) or the finish (true) writes per stream: (n_new, n_emit)
int online_plan(const repet_online* o, int64_t n, bool finishing, int64_t* n_new, int64_t* n_emit) {
    if (o->finished) return fail(REPET_ERR_BAD_ARG, "online: stream already finished");
    if (finishing) {
        const int64_t N = o->total_in;
        if (N < (int64_t)(o->M - 2) * o->H + o->W)      // the warm-up needs M-1 whole frames (the reference's, M = B: repet.py:795-810)
            return fail(REPET_ERR_TOO_SHORT, "operands could not be broadcast together (signal shorter than the buffer)");
        const int64_t T = repet_frame_count(N, o->W, o->H, 0);                   // repet.py:781, last frame zero-padded
        *n_new = std::max<int64_t>(T - o->frames_done, 0);
        *n_emit = N - o->emitted;                                                 // truncate to the samples pushed
        return REPET_OK;
    }
    if (n < 0) return fail(REPET_ERR_BAD_ARG, "bad size");
    const int64_t total = o->total_in + n;
    const int64_t full = total >= o->W ? (total - o->W) / o->H + 1 : 0;          // frames completely covered
    *n_new = std::max<int64_t>(full - o->frames_done, 0);
    *n_emit = *n_new * (int64_t)o->H;
    return REPET_OK;
}

// the chunk's samples (already where `src` says, device memory) appended to every stream's pending buffer
int online_append(repet_online* o, const void* src, int dtype, int64_t n, const int64_t strides[3]) {
    if (n <= 0) return REPET_OK;
    online_invalidate_records(o);
    RP_TRY(online_ensure_pending(o, n));
    hipError_t e = launch_stream_append(src, dtype, o->S, n, o->C, strides, o->pend[o->pcur].as<float>(), o->pend_lo[o->pcur].as<float>(),
                                        o->pend_stride(), (o->pend_hist + o->pend_count) * o->C, o->ctx->stream);
    HIP_TRY(e);
    o->pend_count += n;
    o->total_in += n;
    return REPET_OK;
}

// The last emission (o->em) into up to two strided device destinations of one dtype: one launch. The background alone takes the
// plain egress it always took; everything else reads the emitted range of the pending samples beside the result.
int online_emit(repet_online* o, const EmitDst* dsts, int n_dsts, int dtype) {
    repet_ctx* c = o->ctx;
    const repet_online::Emission& em = o->em;
    if (!em.valid) return fail(REPET_ERR_BAD_ARG, "online: no emission to return");
    if ((int64_t)em.S * em.n * o->C <= 0 || n_dsts <= 0) return REPET_OK;
    // (a held slot's last masked spectrum still rings into the first hop of a push: its background is zeroed with the table, below)
    if (n_dsts == 1 && dsts[0].which == REPET_OUT_BACKGROUND && !(o->n_held > 0 && em.slot < 0)) {
        HIP_TRY(launch_stream_egress(o->outf.as<float>(), em.S, em.n, o->C, dsts[0].p, dtype, dsts[0].strides, c->stream));
        return REPET_OK;
    }
    if (em.off + em.n > o->pend_cap) return fail(REPET_ERR_LIMIT, "online: the emitted range is not in the pending buffer");
    const int64_t sb = em.slot < 0 ? 0 : em.slot, at = sb * o->pend_stride() + em.off * o->C;
    EmitGain gain;
    if (o->gains_on) { gain.a_cur = o->gain_current(em.g0) + sb; gain.a_tgt = o->gain_current(em.g1) + sb; gain.ramp = em.ramp; }
    HIP_TRY(launch_stream_emit(o->outf.as<float>(), o->pend[em.buf].as<float>() + at, o->pend_lo[em.buf].as<float>() + at, o->pend_stride(),
                               o->slots_on ? o->slot_start.as<int64_t>() + sb : nullptr, em.pos0, o->H, em.S, em.n, o->C, dtype, dsts,
                               n_dsts, c->stream, o->gains_on ? &gain : nullptr, em.shaped ? o->outs.as<float>() : nullptr));
    return REPET_OK;
}

// The level record of the last emission (o->em) into dst, dense float64 [em.S][C][REPET_LEVEL_FIELDS] on the device: the
// arguments online_emit gives the emission kernel, so the gain and fade are the emission's own. Enqueues only (one launch, two
// for an emission of several chunks); an empty emission is a memset.
static int online_levels(repet_online* o, double* dst) {
    repet_ctx* c = o->ctx;
    const repet_online::Emission& em = o->em;
    if (!em.valid) return fail(REPET_ERR_BAD_ARG, "online: no emission to measure");
    const bool empty = (int64_t)em.S * em.n * o->C <= 0;
    if (!empty && em.off + em.n > o->pend_cap) return fail(REPET_ERR_LIMIT, "online: the emitted range is not in the pending buffer");
    const int64_t sb = em.slot < 0 ? 0 : em.slot, at = sb * o->pend_stride() + em.off * o->C;
    const int64_t partials = stream_levels_partials(em.S, em.n, o->C);
    if (partials > 0) HIP_TRY(c->levels_ws.ensure((size_t)partials * sizeof(double)));
    EmitGain gain;
    if (o->gains_on) { gain.a_cur = o->gain_current(em.g0) + sb; gain.a_tgt = o->gain_current(em.g1) + sb; gain.ramp = em.ramp; }
    const hipError_t e = launch_stream_levels(o->outf.as<float>(), empty ? nullptr : o->pend[em.buf].as<float>() + at,
                                              empty ? nullptr : o->pend_lo[em.buf].as<float>() + at, o->pend_stride(),
                                              o->slots_on ? o->slot_start.as<int64_t>() + sb : nullptr, em.pos0, o->H, em.S, em.n, o->C, dst,
                                              partials > 0 ? c->levels_ws.as<double>() : nullptr, c->stream, o->gains_on ? &gain : nullptr,
                                              em.shaped ? o->outs.as<float>() : nullptr);
    if (e == hipErrorNotSupported) return fail(REPET_ERR_LIMIT, "too many channels for the level reduction");
    HIP_TRY(e);
    return REPET_OK;
}

// finish_stream is about to drop its slot's samples: on a handle that has been asked for levels, the tail is measured now.
// (A tail the pending buffer no longer holds is not measured: last_levels then refuses as last_emission does.)
static int online_keep_tail_levels(repet_online* o, bool* kept) {
    *kept = false;
    if (!o->levels_on || !o->em.valid || o->em.off + o->em.n > o->pend_cap) return REPET_OK;
    HIP_TRY(o->levels.ensure((size_t)o->C * REPET_LEVEL_FIELDS * sizeof(double)));
    RP_TRY(online_levels(o, o->tail_levels()));
    *kept = true;
    return REPET_OK;
}

// the handle's selected output, and the second one where repet_online_also_emit armed it
static int online_outputs(const repet_online* o, void* dst, const int64_t* strides, void* also_dst, const int64_t* also_strides, EmitDst d[2]) {
    d[0].p = dst; d[0].which = o->out_which;
    for (int k = 0; k < 3; ++k) d[0].strides[k] = strides[k];
    if (o->also.which < 0) return 1;
    d[1].p = also_dst; d[1].which = o->also.which;
    for (int k = 0; k < 3; ++k) d[1].strides[k] = also_strides[k];
    return 2;
}

// host side of a push or finish: the result [S][n_emit][C] widened on the device (two blocks with a second output), one copy
// into the pinned buffer, then `out` (and the second host array)
int online_host_result(repet_online* o, int64_t n_emit, double* out, int streams = 0) {
    repet_ctx* c = o->ctx;
    const int S = streams > 0 ? streams : o->S;
    const int64_t count = (int64_t)S * n_emit * o->C;
    const int blocks = o->also.which < 0 ? 1 : 2;
    if (count <= 0) {                                   // nothing to copy: the call still returns behind its launches
        HIP_TRY(hipStreamSynchronize(c->stream));
        return REPET_OK;
    }
    HIP_TRY(o->out64.ensure((size_t)count * blocks * sizeof(double)));
    const int64_t dense[3] = {n_emit * o->C, o->C, 1};
    EmitDst d[2];
    const int nd = online_outputs(o, o->out64.p, dense, o->out64.as<double>() + count, dense, d);
    RP_TRY(online_emit(o, d, nd, REPET_F64));
    RP_TRY(online_download(o, o->out64.p, (size_t)count * blocks * sizeof(double)));
    std::memcpy(out, o->host_out, (size_t)count * sizeof(double));
    if (blocks == 2) std::memcpy(o->also.dst, static_cast<double*>(o->host_out) + count, (size_t)count * sizeof(double));
    return REPET_OK;
}

// device side: the result into the caller's strided destination(s), then the caller's stream behind it
int online_device_result(repet_online* o, int64_t n_emit, void* dst, int dst_dtype, const int64_t dst_strides[3], void* signal_stream,
                         int streams = 0) {
    EmitDst d[2];
    const int64_t also_strides[3] = {streams > 0 ? 0 : o->also.strides[0], o->also.strides[1], o->also.strides[2]};
    const int nd = online_outputs(o, dst, dst_strides, o->also.dst, also_strides, d);
    RP_TRY(online_emit(o, d, nd, dst_dtype));
    return signal_caller(o->ctx, signal_stream);
}

// the armed second output is consumed by the emitting call that follows it, whether that call succeeds or not
struct AlsoScope {
    repet_online* o;
    explicit AlsoScope(repet_online* h) : o(h) {}
    ~AlsoScope() { if (o) o->also.which = -1; }
};

// the second destination against the call that is about to emit (before any launch): host calls take a dense float64 array
int online_check_also_host(const repet_online* o, int64_t n_emit, const double* out, int streams = 0) {
    if (o->also.which < 0) return REPET_OK;
    if (o->also.dtype != REPET_F64) return fail(REPET_ERR_BAD_ARG, "online: the second output of a host call is float64");
    const int S = streams > 0 ? streams : o->S;
    const int64_t dense[3] = {n_emit * o->C, o->C, 1};
    return check_disjoint(out, dense, o->also.dst, dense, 8, S, n_emit, o->C);
}

int online_check_dst(const repet_online* o, int64_t n_emit, const void* dst, int dst_dtype, const int64_t dst_strides[3], int streams = 0) {
    RP_TRY(check_emit_dtype(dst_dtype));
    RP_TRY(check_strides(dst_strides));
    RP_TRY(check_no_overlap(dst_strides, streams > 0 ? streams : o->S, n_emit, o->C));
    if (n_emit > 0 && !dst) return fail(REPET_ERR_BAD_ARG, "null destination");
    if (o->also.which >= 0) {
        if (n_emit > 0 && !o->also.dst) return fail(REPET_ERR_BAD_ARG, "null destination");
        const int S = streams > 0 ? streams : o->S;
        const int64_t st[3] = {streams > 0 ? 0 : o->also.strides[0], o->also.strides[1], o->also.strides[2]};
        if (o->also.dtype != dst_dtype) return fail(REPET_ERR_BAD_ARG, "online: the two outputs of one call have one dtype");
        RP_TRY(check_strides(st));
        RP_TRY(check_no_overlap(st, S, n_emit, o->C));
        RP_TRY(check_disjoint(dst, dst_strides, o->also.dst, st, dtype_bytes(dst_dtype), S, n_emit, o->C));
    }
    return REPET_OK;
}

// Where the result of an emitting call goes, which is all that tells its host form from its device form: a dense float64 host
// array of `capacity` samples per stream and channel, or strided device memory of `dtype` that `signal_stream` goes on to use.
struct Sink {
    bool device = false;
    double* out = nullptr; int64_t capacity = 0;
    void* dst = nullptr; int dtype = REPET_F64; const int64_t* strides = nullptr; void* signal_stream = nullptr;
};

static Sink host_sink(double* out, int64_t capacity) {
    Sink k;
    k.out = out; k.capacity = capacity;
    return k;
}

static Sink device_sink(void* dst, int dtype, const int64_t* strides, void* signal_stream) {
    Sink k;
    k.device = true; k.dst = dst; k.dtype = dtype; k.strides = strides; k.signal_stream = signal_stream;
    return k;
}

// before any launch: the destination(s) against what the call is about to emit (too_small: the call's own words for a short host array)
static int sink_check(const repet_online* o, const Sink& k, int64_t n_emit, const char* too_small, int streams = 0) {
    if (k.device) return online_check_dst(o, n_emit, k.dst, k.dtype, k.strides, streams);
    if (n_emit > k.capacity || (n_emit > 0 && !k.out)) return fail(REPET_ERR_BAD_ARG, too_small);
    return online_check_also_host(o, n_emit, k.out, streams);
}

// the engine's stream behind what the caller's stream(s) have enqueued so far (the producer of a chunk, earlier users of dst)
static int sink_begin(repet_online* o, const Sink& k, void* wait_stream) {
    return k.device ? wait_caller(o->ctx, wait_stream, k.signal_stream) : REPET_OK;
}

static int sink_deliver(repet_online* o, const Sink& k, int64_t n_emit, int streams = 0) {
    if (k.device) return online_device_result(o, n_emit, k.dst, k.dtype, k.strides, k.signal_stream, streams);
    return online_host_result(o, n_emit, k.out, streams);
}

// The Sink's counterpart for the read-back calls (last_emission, last_levels, last_frames, last_band_energies, last_matches, export,
// import): where a record goes, which again is all that tells the host form from the device form. `n` host arrays of `capacity`
// elements (or rows) each, or `n` device pointers that `stream`, the caller's, goes on to use. An import reads part[0] instead.
struct Reader {
    bool device = false;
    int n = 1;
    void* part[3] = {nullptr, nullptr, nullptr};
    int64_t capacity = 0;
    void* stream = nullptr;
};

static Reader host_reader(void* out, int64_t capacity) { return Reader{false, 1, {out}, capacity, nullptr}; }
static Reader device_reader(void* dst, void* stream) { return Reader{true, 1, {dst}, 0, stream}; }

// before any launch: every part is there, and a host array holds `count` elements
static int read_check(const Reader& r, int64_t count) {
    bool bad = !r.device && r.capacity < count;
    for (int k = 0; k < r.n; ++k) bad = bad || !r.part[k];
    return bad ? fail(REPET_ERR_BAD_ARG, r.device ? "null destination" : "online: output capacity too small") : REPET_OK;
}

// Before the launch: the engine's stream behind what the caller's has enqueued so far (earlier users of the destination), and where
// the launch writes its parts of bytes[k]: the caller's memory, or one block of the handle's that read_deliver takes apart.
static int read_begin(repet_online* o, const Reader& r, const size_t* bytes, void** at) {
    size_t total = 0, off = 0;
    for (int k = 0; k < r.n; ++k) total += bytes[k];
    if (r.device) RP_TRY(wait_caller(o->ctx, r.stream, r.stream));
    else HIP_TRY(o->out64.ensure(total));
    for (int k = 0; k < r.n; off += bytes[k++]) at[k] = r.device ? r.part[k] : o->out64.as<char>() + off;
    return REPET_OK;
}

// Behind the launch: the caller's stream, or one pinned round trip of the block (the handle's own unless `from` names another) and
// the host arrays out of it.
static int read_deliver(repet_online* o, const Reader& r, const size_t* bytes, const void* from = nullptr) {
    if (r.device) return signal_caller(o->ctx, r.stream);
    size_t total = 0, off = 0;
    for (int k = 0; k < r.n; ++k) total += bytes[k];
    RP_TRY(online_download(o, from ? from : o->out64.p, total));
    for (int k = 0; k < r.n; off += bytes[k++]) std::memcpy(r.part[k], static_cast<char*>(o->host_out) + off, bytes[k]);
    return REPET_OK;
}

// a launch has just written the slot's table entry (restart, release, import): nobody holds it any more, and its inbox is empty
static void online_forget_slot(repet_online* o, int32_t slot) {
    o->caller_held[(size_t)slot] = 0;
    o->starved[(size_t)slot] = 0;
    if (o->feed_cap > 0) { o->q_count[(size_t)slot] = 0; o->q_read[(size_t)slot] = 0; }
}

// restart (first_frame = the handle's next frame) or release (kSlotIdle) of the named slots: one launch writes their first
// frame on the device and clears what the slots hold of an earlier stream -- the history rows of Vn and V, the last masked
// spectrum (the overlap-add tail of the next hop), the pending samples and their remainders. Enqueues only.
int online_reset_slots(repet_online* o, const int32_t* slots, int32_t n, int64_t first_frame) {
    repet_ctx* c = o->ctx;
    online_invalidate_records(o);
    if (n <= 0) return REPET_OK;
    const int64_t FS = o->FS, plane = o->plane(), spec = o->spec_stride(), held = (o->pend_hist + o->pend_count) * o->C;
    ZeroPart parts[kRowCopyParts] = {};
    int n_parts = 0;
    if (o->rows_cap > 0) {
        parts[n_parts++] = ZeroPart{o->Vn[o->cur].as<float>(), o->Hh * FS, 1, 0, o->vn_stride()};
        parts[n_parts++] = ZeroPart{o->V[o->cur].as<float>(), o->Hh * FS, o->C, plane, spec};
        parts[n_parts++] = ZeroPart{o->X[o->cur].as<float>() + 2 * (o->Hh - 1) * FS, 2 * FS, o->C, 2 * plane, 2 * spec};
    }
    if (o->pend_cap > 0 && held > 0) {
        parts[n_parts++] = ZeroPart{o->pend[o->pcur].as<float>(), held, 1, 0, o->pend_stride()};
        parts[n_parts++] = ZeroPart{o->pend_lo[o->pcur].as<float>(), held, 1, 0, o->pend_stride()};
    }
    HIP_TRY(launch_slot_reset(o->slot_start.as<int64_t>(), first_frame, slots, n, parts, n_parts, c->stream));
    for (int32_t k = 0; k < n; ++k) {
        int64_t& st = o->start[(size_t)slots[k]];
        o->n_idle += (first_frame == kSlotIdle ? 1 : 0) - (st == kSlotIdle ? 1 : 0);
        st = first_frame;
        unsigned char& hd = o->held[(size_t)slots[k]];            // (the launch wrote the table: a hold ends here)
        o->n_held -= hd;
        hd = 0;
        online_forget_slot(o, slots[k]);
    }
    if (first_frame != kSlotIdle) o->latest_start = std::max(o->latest_start, first_frame);
    o->slots_on = true;
    return REPET_OK;
}

int online_check_slots(const repet_online* o, const int32_t* slots, int32_t n) {
    if (!o || n < 0 || (n > 0 && !slots)) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (o->finished) return fail(REPET_ERR_BAD_ARG, "online: stream already finished");
    for (int32_t k = 0; k < n; ++k) RP_TRY(check_slot(o, slots[k]));
    return REPET_OK;
}

static const char* const kQueuedEnd =
    "online: the stream still has queued samples (repet_online_pad_feed and the ticks that drain them, or repet_online_clear_feed, come first)";
static const char* const kQueuedPush =
    "online: a push while an inbox holds samples (repet_online_tick consumes them, repet_online_clear_feed drops them)";

// what finish_stream of `slot` writes: the frames still to process and the samples of the tail. The slot's stream is the
// handle's samples [start * H, total_in): it ends where the handle stands, so both numbers are those of the handle's own
// finish; only the length that must cover the buffer is the slot's
int online_plan_slot(const repet_online* o, int32_t slot, int64_t* n_new, int64_t* n_emit) {
    if (!o || !n_new || !n_emit) return fail(REPET_ERR_BAD_ARG, "null argument");
    RP_TRY(online_check_slots(o, &slot, 1));
    const int64_t st = o->start[(size_t)slot];
    if (st == kSlotIdle) return fail(REPET_ERR_BAD_ARG, "online: the slot is idle");
    if (o->feed_cap > 0 && o->q_count[(size_t)slot] > 0) return fail(REPET_ERR_BAD_ARG, kQueuedEnd);
    const int64_t N = o->total_in - st * (int64_t)o->H;
    if (N < (int64_t)(o->M - 2) * o->H + o->W)
        return fail(REPET_ERR_TOO_SHORT, "operands could not be broadcast together (signal shorter than the buffer)");
    return online_plan(o, 0, true, n_new, n_emit);
}

// ---- a slot's stream as a value: repet_online_export_stream / import_stream --------------------------------------------------
// On the hop grid a handle that has seen k >= m hops (m = ceil(W / H) - 1) has transformed k - m frames and holds m * H
// unconsumed samples, so a stream of L samples has AGE L / H - m frames (negative while it is shorter than m hops), and a
// slot's state is what online_reset_slots clears: the Hh history rows of Vn and V, the last masked spectrum, and the held
// samples with their remainders. The payload is that, dense and right-aligned at its full size (zero where the stream is
// younger), at pitches that depend on W, H, B and C alone:
//   Vn [Hh][FS] | V [C][Hh][FS] | X [C][FS] float2 | pend [Hh * H + m * H][C] | pend_lo likewise      (fp32, parts padded to 16 bytes
//   in FRONT of the samples). The header (host side, 96 bytes, little-endian) names the geometry, the parameters the online path
//   reads and the stream's place in time.
constexpr uint32_t kStateMagic = 0x53504552u;        // "REPS"
constexpr uint32_t kStateVersion = 1;
struct StateHeader {
    uint32_t magic, version;
    int32_t W, H, B, C, F, cutoff_bins, sim_distance_frames, sim_number, buffer_frames, flags;
    double sim_threshold;
    int64_t age_frames, length_samples, hist_rows, pending_samples, payload_bytes;
};
static_assert(sizeof(StateHeader) == 96, "the stream state header is 96 bytes");

struct StateLayout { int64_t m, samples, rows, pend_len, vn, v, x, pend, pend_lo, floats; };
static StateLayout state_layout(const repet_online* o) {
    StateLayout l{};
    l.m = ceil_div(o->W, o->H) - 1;
    l.samples = ((int64_t)o->Hh + l.m) * o->H;
    l.rows = (int64_t)o->Hh * o->FS;
    l.pend_len = round_up(l.samples * o->C, 4);
    l.vn = 0;
    l.v = l.vn + round_up(l.rows, 4);
    l.x = l.v + round_up(o->C * l.rows, 4);
    l.pend = l.x + round_up((int64_t)o->C * 2 * o->FS, 4);
    l.pend_lo = l.pend + l.pend_len;
    l.floats = l.pend_lo + l.pend_len;
    return l;
}

static void state_header(const repet_online* o, StateHeader* h) {
    std::memset(h, 0, sizeof(*h));
    h->magic = kStateMagic; h->version = kStateVersion;
    h->W = o->W; h->H = o->H; h->B = o->B; h->C = o->C; h->F = o->F;
    h->cutoff_bins = o->p.cutoff_bins; h->sim_distance_frames = o->p.sim_distance_frames; h->sim_number = o->p.sim_number;
    h->buffer_frames = o->p.buffer_frames; h->flags = o->p.flags; h->sim_threshold = o->p.sim_threshold;
    h->payload_bytes = state_layout(o).floats * (int64_t)sizeof(float);
}

static int64_t clamp_rows(const repet_online* o, int64_t age) { return std::min<int64_t>(std::max<int64_t>(age, 0), o->Hh); }

// the header of slot's stream as it stands (host counters only); refusals before any launch
int online_export_plan(const repet_online* o, int32_t slot, StateHeader* h) {
    RP_TRY(online_check_slots(o, &slot, 1));
    if (o->total_in % o->H)
        return fail(REPET_ERR_BAD_ARG, "online: a stream can only be exported on a hop boundary (samples pushed % step_length == 0)");
    const int64_t st = o->start[(size_t)slot];
    if (st == kSlotIdle) return fail(REPET_ERR_BAD_ARG, "online: the slot is idle");
    const StateLayout l = state_layout(o);
    state_header(o, h);
    const int64_t L = o->total_in - st * (int64_t)o->H;
    h->length_samples = L;
    h->age_frames = L / o->H - l.m;
    h->hist_rows = clamp_rows(o, h->age_frames);
    h->pending_samples = std::min<int64_t>(L, l.m * o->H);
    if (L < 0 || h->hist_rows > o->hist_valid || o->pend_hist + o->pend_count > l.samples)
        return fail(REPET_ERR_LIMIT, "online: the slot's stream does not fit the handle's window");
    return REPET_OK;
}

// one launch: the slot's share of the current window and pending buffers -> payload (device memory of h.payload_bytes)
int online_export(repet_online* o, int32_t slot, const StateHeader& h, float* payload) {
    const StateLayout l = state_layout(o);
    const int64_t FS = o->FS, plane = o->plane(), spec = o->spec_stride(), sb = slot;
    const int64_t held = o->pend_hist + o->pend_count, valid = std::min(h.length_samples, held);
    const bool win = o->rows_cap > 0 && h.hist_rows > 0, smp = o->pend_cap > 0 && valid > 0;
    const int64_t row0 = win ? (o->Hh - h.hist_rows) * FS : l.rows;
    const int64_t off = held * o->C - l.pend_len, below = smp ? l.pend_len - valid * o->C : l.pend_len;
    const SlotMove parts[kRowCopyParts] = {
        {win ? o->Vn[o->cur].as<float>() + sb * o->vn_stride() : nullptr, 0, payload + l.vn, l.rows, 1, 0, 0, row0},
        {win ? o->V[o->cur].as<float>() + sb * spec : nullptr, 0, payload + l.v, l.rows, o->C, plane, l.rows, row0},
        {win ? o->X[o->cur].as<float>() + 2 * (sb * spec + (o->Hh - 1) * FS) : nullptr, 0, payload + l.x, 2 * FS, o->C, 2 * plane, 2 * FS,
         win ? 0 : 2 * FS},
        {smp ? o->pend[o->pcur].as<float>() + sb * o->pend_stride() : nullptr, off, payload + l.pend, l.pend_len, 1, 0, 0, below},
        {smp ? o->pend_lo[o->pcur].as<float>() + sb * o->pend_stride() : nullptr, off, payload + l.pend_lo, l.pend_len, 1, 0, 0, below}};
    HIP_TRY(launch_slot_export(parts, kRowCopyParts, o->ctx->stream));
    return REPET_OK;
}

// everything of a header against the handle and the slot, before any launch
int online_import_check(const repet_online* o, int32_t slot, const StateHeader* h) {
    RP_TRY(online_check_slots(o, &slot, 1));
    if (h->magic != kStateMagic) return fail(REPET_ERR_BAD_ARG, "online: not a stream state (unknown magic word)");
    if (h->version != kStateVersion) return fail(REPET_ERR_BAD_ARG, "online: unknown version of the stream state");
    StateHeader mine;
    state_header(o, &mine);
    if (h->W != mine.W || h->H != mine.H || h->B != mine.B || h->C != mine.C || h->F != mine.F)
        return fail(REPET_ERR_BAD_ARG, "online: the stream state has another geometry (window, hop, buffer, channels) than the handle");
    if (h->cutoff_bins != mine.cutoff_bins || h->sim_distance_frames != mine.sim_distance_frames || h->sim_number != mine.sim_number ||
        h->buffer_frames != mine.buffer_frames || h->flags != mine.flags || std::memcmp(&h->sim_threshold, &mine.sim_threshold, sizeof(double)))
        return fail(REPET_ERR_BAD_ARG, "online: the stream state was made with other parameters than the handle's");
    if (h->payload_bytes != mine.payload_bytes) return fail(REPET_ERR_BAD_ARG, "online: the stream state has another payload size");
    const StateLayout l = state_layout(o);
    const int64_t L = h->length_samples;
    if (L < 0 || L % o->H || h->age_frames != L / o->H - l.m || h->hist_rows != clamp_rows(o, h->age_frames) ||
        h->pending_samples != std::min<int64_t>(L, l.m * o->H))
        return fail(REPET_ERR_BAD_ARG, "online: the stream state's age, length and held counts contradict each other");
    if (o->total_in % o->H)
        return fail(REPET_ERR_BAD_ARG, "online: a stream can only be imported on a hop boundary (samples pushed % step_length == 0)");
    return REPET_OK;
}

// The handle read as if it had been opened `delta` hops earlier, with every live slot idle until its own start: the counters
// move by delta hops (frames done and held samples as a handle of that age has them), every live slot's first frame moves with
// them (the device table: by the import launch that follows), and the held samples of every slot move behind delta * H zeros
// -- the samples before their starts -- into the other pending buffer: one launch. The history rows this exposes were never
// written (zeroed at allocation, kept so by the slide and the resets). Only while the handle is younger than B - 1 frames, whatever start_frames is: a slot's own
// frame numbers do not move with the epoch, so its young rows (from its frame M - 1 on) are the same rows before and after.
static int online_shift_epoch(repet_online* o, int64_t delta) {
    repet_ctx* c = o->ctx;
    const int64_t by = delta * o->H, old_held = o->pend_hist + o->pend_count;
    const int64_t total = o->total_in + by;
    const int64_t frames = total >= o->W ? (total - o->W) / o->H + 1 : 0;
    const int64_t hist = std::min<int64_t>(o->Hh, frames);
    const int64_t count = total - frames * (int64_t)o->H;
    if (o->frames_done != o->hist_valid || frames != hist || hist * o->H + count != old_held + by || old_held + by > o->pend_cap)
        return fail(REPET_ERR_LIMIT, "online: the handle is too old for an epoch shift");
    const int64_t pst = o->pend_stride(), lead = by * o->C, len = old_held * o->C;
    const int nxt = o->pcur ^ 1;
    const RowCopy parts[4] = {{nullptr, o->pend[nxt].as<float>(), lead, 1, 0, 0, 0, pst},
                              {nullptr, o->pend_lo[nxt].as<float>(), lead, 1, 0, 0, 0, pst},
                              {o->pend[o->pcur].as<float>(), o->pend[nxt].as<float>() + lead, len, 1, 0, 0, pst, pst},
                              {o->pend_lo[o->pcur].as<float>(), o->pend_lo[nxt].as<float>() + lead, len, 1, 0, 0, pst, pst}};
    HIP_TRY(launch_row_copies(parts, 4, o->S, c->stream));
    o->pcur = nxt;
    o->total_in = total; o->frames_done = frames; o->hist_valid = hist; o->pend_hist = hist * o->H; o->pend_count = count;
    o->emitted = frames * (int64_t)o->H;
    for (int64_t& st : o->start)
        if (st != kSlotIdle) st += delta;
    o->latest_start += delta;
    o->epoch += delta;
    o->slots_on = true;
    return REPET_OK;
}

// the checked state into `slot` (payload: device memory on the handle's device). The stream's frame `age` is the handle's next
// frame: start[slot] = frames_done - age, negative for a stream older than the handle. A handle too young to hold the state
// (fewer frames done than the state has history rows, or fewer held samples) is first moved back in time (online_shift_epoch).
// One launch writes everything online_reset_slots clears, and the table.
int online_import(repet_online* o, int32_t slot, const StateHeader& h, const float* payload) {
    repet_ctx* c = o->ctx;
    const StateLayout l = state_layout(o);
    const int64_t delta = std::max<int64_t>(0, l.m + h.hist_rows - o->total_in / o->H);
    online_invalidate_records(o);
    RP_TRY(online_ensure_windows(o, std::max<int64_t>(o->max_push / o->H + 1, o->W / o->H + 1)));
    RP_TRY(online_ensure_pending(o, delta * o->H));
    if (delta > 0) RP_TRY(online_shift_epoch(o, delta));
    const int64_t FS = o->FS, plane = o->plane(), spec = o->spec_stride(), sb = slot;
    const int64_t held = o->pend_hist + o->pend_count;
    if (o->rows_cap < o->Hh || h.hist_rows > o->hist_valid || held > l.samples || held > o->pend_cap || o->pend_count != l.m * o->H)
        return fail(REPET_ERR_LIMIT, "online: the stream state does not fit the handle's window");
    const int64_t off = l.pend_len - held * o->C;
    const SlotMove parts[kRowCopyParts] = {
        {payload + l.vn, 0, o->Vn[o->cur].as<float>() + sb * o->vn_stride(), l.rows, 1, 0, 0, 0},
        {payload + l.v, 0, o->V[o->cur].as<float>() + sb * spec, l.rows, o->C, l.rows, plane, 0},
        {payload + l.x, 0, o->X[o->cur].as<float>() + 2 * (sb * spec + (o->Hh - 1) * FS), 2 * FS, o->C, 2 * FS, 2 * plane, 0},
        {payload + l.pend, off, o->pend[o->pcur].as<float>() + sb * o->pend_stride(), held * o->C, 1, 0, 0, 0},
        {payload + l.pend_lo, off, o->pend_lo[o->pcur].as<float>() + sb * o->pend_stride(), held * o->C, 1, 0, 0, 0}};
    const int64_t first = o->frames_done - h.age_frames;
    HIP_TRY(launch_slot_import(parts, kRowCopyParts, o->slot_start.as<int64_t>(), o->S, slot, first, delta, c->stream));
    int64_t& st = o->start[(size_t)slot];
    if (st == kSlotIdle) o->n_idle -= 1;
    st = first;
    o->n_held -= o->held[(size_t)slot];                         // (the launch wrote the table: a hold ends here)
    o->held[(size_t)slot] = 0;
    online_forget_slot(o, slot);
    if (o->bands_on && o->band_stale[(size_t)slot]) {
        // band gains: the frame that comes with the stream is shaped with the table the slot has now
        HIP_TRY(launch_band_commit(o->band_tab.as<float>(), o->FS, o->S, slot, kBandSettle, nullptr, c->stream));
        o->band_mark((size_t)slot, 0, (o->band_nd[(size_t)slot] & 1) ? 7 : 0);
    }
    o->latest_start = std::max(o->latest_start, first);
    o->slots_on = true;
    return REPET_OK;
}

// The device table follows the flags of the named slots: a slot is held on the device while the caller holds it (caller_held) or
// a tick found its inbox short (starved). One small launch writes kSlotHeld, or the slots' own first frames again, for the slots
// whose state changes; with none nothing is enqueued and nothing changes. Enqueues only.
static int online_sync_holds(repet_online* o, const int32_t* slots, int32_t n) {
    repet_ctx* c = o->ctx;
    std::vector<int32_t> ids;
    std::vector<int64_t> values;
    for (int32_t k = 0; k < n; ++k) {
        const size_t s = (size_t)slots[k];
        const bool want = o->caller_held[s] || o->starved[s];
        unsigned char& hd = o->held[s];
        if ((hd != 0) == want) continue;
        hd = want ? 1 : 0;
        o->n_held += want ? 1 : -1;
        ids.push_back(slots[k]);
        values.push_back(want ? kSlotHeld : o->start[s]);
    }
    if (ids.empty()) return REPET_OK;
    online_invalidate_records(o);
    o->slots_on = true;
    HIP_TRY(launch_slot_set(o->slot_start.as<int64_t>(), ids.data(), values.data(), (int32_t)ids.size(), c->stream));
    return REPET_OK;
}

// Hold (on = true) or resume the named slots for the caller. Slots that are there already are skipped, and so is the resume of
// a starved slot, which stays held on the device until a tick finds it ready. end_starved: the call ends that too (finish and
// finish_stream, which end the slots as they stand).
int online_hold_slots(repet_online* o, const int32_t* slots, int32_t n, bool on, bool end_starved = false) {
    for (int32_t k = 0; k < n; ++k) {
        o->caller_held[(size_t)slots[k]] = on ? 1 : 0;
        if (end_starved) o->starved[(size_t)slots[k]] = 0;
    }
    return online_sync_holds(o, slots, n);
}

// finish and finish_stream end the holds of the slots they end
int online_resume_all(repet_online* o) {
    if (o->n_held == 0) return REPET_OK;
    std::vector<int32_t> ids;
    for (int32_t s = 0; s < o->S; ++s)
        if (o->held[(size_t)s]) ids.push_back(s);
    return online_hold_slots(o, ids.data(), (int32_t)ids.size(), false, true);
}

// ---- per-slot inboxes: repet_online_enable_feed / feed / tick ----------------------------------------------------------------
static const char* const kNoFeed = "online: the handle has no inboxes (repet_online_enable_feed comes first)";

static int online_check_feed(const repet_online* o) {
    if (!o) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (o->feed_cap <= 0) return fail(REPET_ERR_BAD_ARG, kNoFeed);
    if (o->finished) return fail(REPET_ERR_BAD_ARG, "online: stream already finished");
    return REPET_OK;
}

// whether any inbox holds samples (never on a handle without inboxes)
static bool online_any_queued(const repet_online* o) {
    if (o->feed_cap <= 0) return false;
    for (int64_t q : o->q_count)
        if (q > 0) return true;
    return false;
}

// the slots the caller holds: what the whole-hop rule of a push counts (starved slots are resumed by the push itself)
static int64_t online_caller_holds(const repet_online* o) {
    if (o->feed_cap <= 0) return o->n_held;
    int64_t n = 0;
    for (unsigned char h : o->caller_held) n += h;
    return n;
}

// a plain push after ticks: nobody is starved any more (one launch per 256 slots that were, none where no slot is)
static int online_end_starving(repet_online* o) {
    if (o->feed_cap <= 0) return REPET_OK;
    std::vector<int32_t> ids;
    for (int32_t s = 0; s < o->S; ++s)
        if (o->starved[(size_t)s]) { o->starved[(size_t)s] = 0; ids.push_back(s); }
    return online_sync_holds(o, ids.data(), (int32_t)ids.size());
}

// the checked rows of a feed: slot ids, counts and the ring positions they are written from; then the host counters move
struct FeedPlan { std::vector<int32_t> slots; std::vector<int64_t> counts, wpos; };

static int online_feed_plan(const repet_online* o, const int32_t* slots, const int64_t* counts, int32_t n_slots, int64_t n, FeedPlan* plan) {
    RP_TRY(online_check_feed(o));
    if (n_slots < 0 || n < 0 || (n_slots > 0 && !slots)) return fail(REPET_ERR_BAD_ARG, "bad size");
    std::vector<unsigned char> seen((size_t)o->S, 0);
    for (int32_t k = 0; k < n_slots; ++k) {
        const int32_t s = slots[k];
        RP_TRY(check_slot(o, s));
        if (seen[(size_t)s]) return fail(REPET_ERR_BAD_ARG, "online: a slot is named twice in one feed");
        seen[(size_t)s] = 1;
        if (o->start[(size_t)s] == kSlotIdle) return fail(REPET_ERR_BAD_ARG, "online: the slot is idle");
        const int64_t cnt = counts ? counts[k] : n;
        if (cnt < 0 || cnt > n) return fail(REPET_ERR_BAD_ARG, "online: a count of a feed lies in [0, n]");
        if (o->q_count[(size_t)s] + cnt > o->feed_cap) return fail(REPET_ERR_BAD_ARG, "online: the inbox of a slot would overflow (its capacity is enable_feed's)");
        plan->slots.push_back(s);
        plan->counts.push_back(cnt);
        plan->wpos.push_back(((o->q_read[(size_t)s] + o->q_count[(size_t)s]) % o->feed_cap) * o->C);
    }
    return REPET_OK;
}

static int online_feed_launch(repet_online* o, const FeedPlan& plan, const void* src, int dtype, int64_t n, const int64_t strides[3]) {
    HIP_TRY(launch_feed(src, dtype, n, o->C, strides, plan.slots.data(), plan.counts.data(), plan.wpos.data(), (int32_t)plan.slots.size(),
                        o->ring_hi(), o->ring_lo(), o->ring_stride, o->feed_cap * o->C, o->ctx->stream));
    for (size_t k = 0; k < plan.slots.size(); ++k) o->q_count[(size_t)plan.slots[k]] += plan.counts[k];
    return REPET_OK;
}

// A tick's plan, from the host counters alone: who is ready (live, not held by the caller, hops * H samples queued), and what the
// push of hops * H samples completes and emits. Nobody ready: *n_ready = 0 and the tick is not made.
static int online_tick_plan(const repet_online* o, int64_t hops, std::vector<unsigned char>* ready, int64_t* n_ready, int64_t* n,
                            int64_t* n_new, int64_t* n_emit) {
    RP_TRY(online_check_feed(o));
    if (hops < 1 || hops > INT32_MAX) return fail(REPET_ERR_BAD_ARG, "online: a tick is at least one hop");
    if (o->total_in % o->H) return fail(REPET_ERR_BAD_ARG, "online: a tick is only made on a hop boundary (samples pushed % step_length == 0)");
    *n = hops * (int64_t)o->H;
    ready->assign((size_t)o->S, 0);
    *n_ready = 0;
    for (size_t s = 0; s < (size_t)o->S; ++s)
        if (o->start[s] != kSlotIdle && !o->caller_held[s] && o->q_count[s] >= *n) { (*ready)[s] = 1; *n_ready += 1; }
    return online_plan(o, *n, false, n_new, n_emit);
}

// The tick's chunk: the slots that are short are starved and those that were and are ready again resumed (the table changes only
// where a slot's state does: a slot the caller holds keeps its flag until it is looked at again), then the ready slots' oldest
// n samples go from their rings to where a push's append would have put them, and leave the queues.
static int online_tick_take(repet_online* o, const std::vector<unsigned char>& ready, int64_t n) {
    repet_ctx* c = o->ctx;
    std::vector<int32_t> changed;
    for (int32_t s = 0; s < o->S; ++s) {
        const size_t k = (size_t)s;
        if (o->start[k] == kSlotIdle || o->caller_held[k]) continue;
        const unsigned char want = ready[k] ? 0 : 1;
        if (o->starved[k] == want) continue;
        o->starved[k] = want;
        changed.push_back(s);
    }
    RP_TRY(online_sync_holds(o, changed.data(), (int32_t)changed.size()));
    online_invalidate_records(o);
    RP_TRY(online_ensure_pending(o, n));
    std::vector<int64_t> rpos((size_t)o->S);
    for (size_t s = 0; s < (size_t)o->S; ++s) rpos[s] = o->q_read[s] * o->C;
    HIP_TRY(launch_take(o->ring_hi(), o->ring_lo(), o->ring_stride, o->feed_cap * o->C, rpos.data(), o->S, n * o->C,
                        o->pend[o->pcur].as<float>(), o->pend_lo[o->pcur].as<float>(), o->pend_stride(),
                        (o->pend_hist + o->pend_count) * o->C, o->slot_start.as<int64_t>(), c->stream));
    o->pend_count += n;
    o->total_in += n;
    for (size_t s = 0; s < (size_t)o->S; ++s)
        if (ready[s]) { o->q_count[s] -= n; o->q_read[s] = (o->q_read[s] + n) % o->feed_cap; }
    return REPET_OK;
}

// ---- the emitting calls: one body each for the host and the device form (the public entry points build the Sink) -----------------
// Every refusal comes before the first launch, in the order a caller of either form has always seen. *n_written is zero from the
// point each body says and the count of the emission on success alone.
static const char* const kHeldPush = "online: while a stream is held a push is a whole number of hops (n % step_length == 0)";

// A host chunk (k.device false) is dense [S][n][C] of a dtype up to REPET_I16 and goes through the pinned buffer; a device chunk
// lies at src_strides, of a dtype up to REPET_BF16, produced on wait_stream.
static int online_push_impl(repet_online* o, const void* src, int dtype, int64_t n, const int64_t* src_strides, void* wait_stream,
                            const Sink& k, int64_t* n_written) {
    if (!o || !n_written || (n > 0 && !src)) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (o->finished) return fail(REPET_ERR_BAD_ARG, "online: stream already finished");
    if (n < 0 || dtype < REPET_F32 || dtype > (k.device ? REPET_BF16 : REPET_I16)) return fail(REPET_ERR_BAD_ARG, "bad size or dtype");
    if (online_any_queued(o)) return fail(REPET_ERR_BAD_ARG, kQueuedPush);
    if (online_caller_holds(o) > 0 && n % o->H) return fail(REPET_ERR_BAD_ARG, kHeldPush);
    if (k.device) RP_TRY(check_strides(src_strides));
    *n_written = 0;
    int64_t n_new = 0, n_emit = 0;
    RP_TRY(online_plan(o, n, false, &n_new, &n_emit));
    RP_TRY(sink_check(o, k, n_emit, "online: output capacity too small (needs n_samples + window_length)"));
    DeviceGuard guard(o->ctx->device);
    RP_TRY(sink_begin(o, k, wait_stream));
    RP_TRY(online_end_starving(o));                             // (after ticks: the slots they starved take part again)
    const int64_t dense[3] = {n * o->C, o->C, 1};
    if (!k.device && n > 0) {
        // the chunk [S][n][C] through the pinned buffer into the staging buffer, then appended to every stream on the device
        const size_t esz = dtype == REPET_F64 ? 8 : (dtype == REPET_F32 ? 4 : 2);
        RP_TRY(online_upload(o, src, (size_t)o->S * n * o->C * esz));
        src = o->staging.p;
    }
    RP_TRY(online_append(o, src, dtype, n, k.device ? src_strides : dense));
    RP_TRY(online_process(o, n_new, n_emit, -1, n));
    RP_TRY(sink_deliver(o, k, n_emit));
    *n_written = n_emit;
    return REPET_OK;
}

static int online_tick_impl(repet_online* o, int64_t hops, const Sink& k, uint8_t* consumed, int64_t* n_written) {
    if (!o || !n_written) return fail(REPET_ERR_BAD_ARG, "null argument");
    *n_written = 0;
    std::vector<unsigned char> ready;
    int64_t n_ready = 0, n = 0, n_new = 0, n_emit = 0;
    RP_TRY(online_tick_plan(o, hops, &ready, &n_ready, &n, &n_new, &n_emit));
    if (n_ready > 0) {                                          // (nobody ready: the tick is not made, and `ready` is all zero)
        RP_TRY(sink_check(o, k, n_emit, "online: output capacity too small (needs hops * step_length)"));
        DeviceGuard guard(o->ctx->device);
        RP_TRY(sink_begin(o, k, k.signal_stream));
        RP_TRY(online_tick_take(o, ready, n));
        RP_TRY(online_process(o, n_new, n_emit, -1, n));
        RP_TRY(sink_deliver(o, k, n_emit));
        *n_written = n_emit;
    }
    if (consumed) std::copy(ready.begin(), ready.end(), consumed);
    return REPET_OK;
}

static int online_finish_impl(repet_online* o, const Sink& k, int64_t* n_written) {
    if (!o || !n_written) return fail(REPET_ERR_BAD_ARG, "null argument");
    *n_written = 0;
    int64_t n_new = 0, n_emit = 0;
    RP_TRY(online_plan(o, 0, true, &n_new, &n_emit));
    if (online_any_queued(o)) return fail(REPET_ERR_BAD_ARG, kQueuedEnd);
    RP_TRY(sink_check(o, k, n_emit, "online: output capacity too small"));
    DeviceGuard guard(o->ctx->device);
    RP_TRY(sink_begin(o, k, k.signal_stream));
    RP_TRY(online_resume_all(o));                               // held slots end as they stand, each with its own length
    RP_TRY(online_process(o, n_new, n_emit));
    RP_TRY(sink_deliver(o, k, n_emit));
    *n_written = n_emit;
    o->finished = true;
    return REPET_OK;
}

// (streams = 1 throughout: the result is the one slot's, [n_emit][C], and a device sink's strides begin with a 0)
static int online_finish_stream_impl(repet_online* o, int32_t slot, const Sink& k, int64_t* n_written) {
    if (!o || !n_written) return fail(REPET_ERR_BAD_ARG, "null argument");
    *n_written = 0;
    int64_t n_new = 0, n_emit = 0;
    RP_TRY(online_plan_slot(o, slot, &n_new, &n_emit));
    RP_TRY(sink_check(o, k, n_emit, "online: output capacity too small", 1));
    DeviceGuard guard(o->ctx->device);
    o->slots_on = true;
    RP_TRY(sink_begin(o, k, k.signal_stream));
    RP_TRY(online_hold_slots(o, &slot, 1, false, true));        // a held slot ends as it stands
    RP_TRY(online_process(o, n_new, n_emit, slot));
    RP_TRY(sink_deliver(o, k, n_emit, 1));
    // the call drops its slot's samples: the tail's levels are measured first, and their record outlives the reset
    bool kept = false;
    RP_TRY(online_keep_tail_levels(o, &kept));
    RP_TRY(online_reset_slots(o, &slot, 1, kSlotIdle));
    o->tail_valid = kept;
    *n_written = n_emit;
    return REPET_OK;
}

}  // namespace repet_eng

extern "C" {

static int check_which(int which) {
    if (which < REPET_OUT_BACKGROUND || which > REPET_OUT_MIXTURE)
        return fail(REPET_ERR_BAD_ARG, "which must be REPET_OUT_BACKGROUND, REPET_OUT_FOREGROUND or REPET_OUT_MIXTURE");
    return REPET_OK;
}

int repet_online_set_output(repet_online* o, int which) {
    if (!o) return fail(REPET_ERR_BAD_ARG, "null argument");
    RP_TRY(check_which(which));
    o->out_which = which;
    return REPET_OK;
}

int repet_online_also_emit(repet_online* o, int which, void* dst, int dtype, const int64_t strides[3]) {
    if (!o) return fail(REPET_ERR_BAD_ARG, "null argument");
    o->also.which = -1;
    RP_TRY(check_which(which));
    RP_TRY(check_emit_dtype(dtype));
    if (o->finished) return fail(REPET_ERR_BAD_ARG, "online: stream already finished");
    o->also.dst = dst; o->also.dtype = dtype;
    for (int k = 0; k < 3; ++k) o->also.strides[k] = strides ? strides[k] : 0;
    o->also.which = which;
    return REPET_OK;
}

static const char* const kStaleLevels = "online: the last emission is stale (a push, finish, restart or release came after it)";

// ---- the read-back calls: one body each for the host and the device form (the public entry points build the Reader) -------------
// Every refusal comes before the first launch and before the DeviceGuard, per form in the order and with the words its callers have
// always seen; so does what each exit leaves in *n_written / *n_rows. A device form without such a counter passes a local.

// The host form is float64 and dense (dst_strides null); a device destination lies at dst_strides, with stride 0 for the stream axis
// of a finish_stream tail. The device form waits and signals even for an empty emission, the host form does no device work for one.
static int online_read_emission_impl(repet_online* o, int which, const Reader& r, int dtype, const int64_t* dst_strides, int64_t* n_written) {
    if (!o || !n_written) return fail(REPET_ERR_BAD_ARG, "null argument");
    *n_written = 0;
    RP_TRY(check_which(which));
    if (!o->em.valid) return fail(REPET_ERR_BAD_ARG, kStaleLevels);
    const int64_t n = o->em.n, count = (int64_t)o->em.S * n * o->C;
    EmitDst d;
    d.which = which; d.strides[0] = n * o->C; d.strides[1] = o->C; d.strides[2] = 1;
    if (r.device) {
        RP_TRY(check_emit_dtype(dtype));
        RP_TRY(check_strides(dst_strides));
        for (int k = 0; k < 3; ++k) d.strides[k] = k == 0 && o->em.slot >= 0 ? 0 : dst_strides[k];
        RP_TRY(check_no_overlap(d.strides, o->em.S, n, o->C));
        if (count > 0) RP_TRY(read_check(r, count));
    } else if (n > r.capacity || (count > 0 && !r.part[0])) {
        return fail(REPET_ERR_BAD_ARG, "online: output capacity too small");
    }
    DeviceGuard guard(o->ctx->device);
    if (r.device || count > 0) {
        const size_t bytes = (size_t)count * sizeof(double);
        RP_TRY(read_begin(o, r, &bytes, &d.p));
        RP_TRY(online_emit(o, &d, 1, dtype));
        RP_TRY(read_deliver(o, r, &bytes));
    }
    *n_written = n;
    return REPET_OK;
}

int repet_online_last_emission(repet_online* o, int which, double* out, int64_t capacity, int64_t* n_written) {
    return online_read_emission_impl(o, which, host_reader(out, capacity), REPET_F64, nullptr, n_written);
}

int repet_online_last_emission_device(repet_online* o, int which, void* dst, int dst_dtype, const int64_t dst_strides[3],
                                      void* signal_stream, int64_t* n_written) {
    return online_read_emission_impl(o, which, device_reader(dst, signal_stream), dst_dtype, dst_strides, n_written);
}

// float64 [S][C][REPET_LEVEL_FIELDS], dense in either form. A finish_stream tail's record was kept when the call was made and is
// not reduced again: the host form downloads it where it lies, the device form copies it.
static int online_read_levels_impl(repet_online* o, const Reader& r, int64_t* n_written) {
    if (!o || !n_written) return fail(REPET_ERR_BAD_ARG, "null argument");
    *n_written = 0;
    o->levels_on = true;
    if (!o->em.valid && !o->tail_valid) return fail(REPET_ERR_BAD_ARG, kStaleLevels);
    const int64_t count = (int64_t)(o->tail_valid ? 1 : o->em.S) * o->C * REPET_LEVEL_FIELDS;
    *n_written = count;                                         // (a short or null host array is told the count it needs)
    RP_TRY(read_check(r, count));
    *n_written = 0;
    DeviceGuard guard(o->ctx->device);
    const size_t bytes = (size_t)count * sizeof(double);
    void* at = nullptr;
    RP_TRY(read_begin(o, r, &bytes, &at));
    if (!o->tail_valid)
        RP_TRY(online_levels(o, static_cast<double*>(at)));
    else if (r.device)
        HIP_TRY(hipMemcpyAsync(at, o->tail_levels(), bytes, hipMemcpyDeviceToDevice, o->ctx->stream));
    RP_TRY(read_deliver(o, r, &bytes, o->tail_valid ? o->tail_levels() : nullptr));
    *n_written = count;
    return REPET_OK;
}

int repet_online_last_levels(repet_online* o, double* out, int64_t capacity_doubles, int64_t* n_written) {
    return online_read_levels_impl(o, host_reader(out, capacity_doubles), n_written);
}

int repet_online_last_levels_device(repet_online* o, void* dst, void* signal_stream) {
    int64_t n = 0;
    return online_read_levels_impl(o, device_reader(dst, signal_stream), &n);
}

static const char* const kStaleFrames =
    "online: the last frames are stale (a push, finish, finish_stream, restart, release, import, hold or resume came after them)";

// what the frame kernels read of the last push (o->fr), from the host record alone
static int online_frame_args(const repet_online* o, int which, FrameArgs* a) {
    const repet_online::Frames& fr = o->fr;
    *a = FrameArgs{};
    if (fr.n <= 0) return REPET_OK;
    if (fr.row0 < 0 || fr.row0 + fr.n > o->rows_cap || fr.S != o->S) return fail(REPET_ERR_LIMIT, "online: the last frames are not in the window");
    const int64_t at = fr.row0 * o->FS;
    a->V = o->V[fr.win].as<float>() + at; a->X = o->X[fr.win].as<float2>() + at;
    a->plane = o->plane(); a->spec = o->spec_stride(); a->FS = o->FS; a->F = o->F; a->C = o->C; a->which = which;
    a->n_frames = fr.n; a->frame0 = fr.first; a->warm = o->M - 1;
    a->slot_start = o->slots_on ? o->slot_start.as<int64_t>() : nullptr;
    return REPET_OK;
}

// n_bands + 1 edges (the caller has checked n_bands against its own limits)
static int check_edges_ascend(const repet_online* o, const int32_t* edges, int32_t n_bands) {
    for (int32_t k = 0; k <= n_bands; ++k)
        if (edges[k] < 0 || edges[k] > o->F || (k > 0 && edges[k] < edges[k - 1]))
            return fail(REPET_ERR_BAD_ARG, "online: band edges are ascending bins in [0, window_length / 2 + 1]");
    return REPET_OK;
}

static int check_band_edges(const repet_online* o, const int32_t* edges, int32_t n_bands) {
    if (n_bands > REPET_MAX_BANDS) return fail(REPET_ERR_LIMIT, "online: at most REPET_MAX_BANDS (128) bands");
    if (n_bands < 1 || !edges) return fail(REPET_ERR_BAD_ARG, "online: at least one band and its edges");
    return check_edges_ascend(o, edges, n_bands);
}

// a destination [S][n][C][F] at element strides: non-negative, and no two elements at one address (check_no_overlap's rule)
static int check_frame_strides(const int64_t* strides, const int64_t size[4]) {
    if (!strides) return fail(REPET_ERR_BAD_ARG, "strides is null");
    int order[4] = {0, 1, 2, 3};
    for (int k = 0; k < 4; ++k)
        if (strides[k] < 0) return fail(REPET_ERR_BAD_ARG, "negative stride (make the tensor contiguous first)");
    std::sort(order, order + 4, [&](int a, int b) { return strides[a] < strides[b]; });
    int64_t span = 0;
    for (int k : order) {
        if (size[k] <= 1) continue;
        if (strides[k] <= span) return fail(REPET_ERR_BAD_ARG, "the destination's elements overlap (an expanded or aliasing view)");
        span += strides[k] * (size[k] - 1);
    }
    return REPET_OK;
}

int repet_online_last_frame_range(repet_online* o, int64_t* first_frame, int64_t* n_frames) {
    if (!o || !first_frame || !n_frames) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (!o->fr.valid) return fail(REPET_ERR_BAD_ARG, kStaleFrames);
    *first_frame = o->fr.first - o->epoch;
    *n_frames = o->fr.n;
    return REPET_OK;
}

// The frames (bands false: float32 [S][n][C][F], at dst_strides on the device and dense on the host) or their band energies
// (float64 [S][n][C][n_bands], dense in either form). An empty record is OK with nothing enqueued: the host form says so before it
// looks at its array, the device form after it has checked its destination.
static int online_read_frames_impl(repet_online* o, int which, bool bands, const int32_t* edges, int32_t n_bands, const Reader& r,
                                   const int64_t* dst_strides, int64_t* n_written) {
    if (!o || !n_written) return fail(REPET_ERR_BAD_ARG, "null argument");
    *n_written = 0;
    RP_TRY(check_which(which));
    if (bands) RP_TRY(check_band_edges(o, edges, n_bands));
    if (!o->fr.valid) return fail(REPET_ERR_BAD_ARG, kStaleFrames);
    const int64_t size[4] = {o->S, o->fr.n, o->C, bands ? n_bands : o->F};
    const int64_t dense[4] = {size[1] * size[2] * size[3], size[2] * size[3], size[3], 1}, count = size[0] * dense[0];
    if (r.device || count > 0) {
        *n_written = count;                                     // (a short or null host array is told the count it needs)
        if (r.device && !bands) RP_TRY(check_frame_strides(dst_strides, size));
        RP_TRY(read_check(r, count));
        *n_written = 0;
    }
    if (count == 0) return REPET_OK;
    FrameArgs a;
    RP_TRY(online_frame_args(o, which, &a));
    DeviceGuard guard(o->ctx->device);
    const size_t bytes = (size_t)count * (bands ? sizeof(double) : sizeof(float));
    void* at = nullptr;
    RP_TRY(read_begin(o, r, &bytes, &at));
    if (bands)
        HIP_TRY(launch_online_bands(a, o->S, edges, n_bands, static_cast<double*>(at), o->ctx->stream));
    else
        HIP_TRY(launch_online_frames(a, o->S, static_cast<float*>(at), r.device ? dst_strides : dense, o->ctx->stream));
    RP_TRY(read_deliver(o, r, &bytes));
    *n_written = count;
    return REPET_OK;
}

int repet_online_last_frames(repet_online* o, int which, float* out, int64_t capacity_floats, int64_t* n_written) {
    return online_read_frames_impl(o, which, false, nullptr, 0, host_reader(out, capacity_floats), nullptr, n_written);
}

int repet_online_last_frames_device(repet_online* o, int which, void* dst, const int64_t dst_strides[4], void* signal_stream) {
    int64_t n = 0;
    return online_read_frames_impl(o, which, false, nullptr, 0, device_reader(dst, signal_stream), dst_strides, &n);
}

int repet_online_last_band_energies(repet_online* o, int which, const int32_t* edges, int32_t n_bands, double* out,
                                    int64_t capacity_doubles, int64_t* n_written) {
    return online_read_frames_impl(o, which, true, edges, n_bands, host_reader(out, capacity_doubles), nullptr, n_written);
}

int repet_online_last_band_energies_device(repet_online* o, int which, const int32_t* edges, int32_t n_bands, void* dst,
                                           void* signal_stream) {
    int64_t n = 0;
    return online_read_frames_impl(o, which, true, edges, n_bands, device_reader(dst, signal_stream), nullptr, &n);
}

static const char* const kStaleMatches =
    "online: the last matches are stale (a push, finish, finish_stream, restart, release, import, hold or resume came after them)";

static int online_max_peaks(const repet_online* o) {
    return (int)std::min<int64_t>(o->p.sim_number, ceil_div(o->B, o->p.sim_distance_frames + 1));
}

// what the match kernel reads of the last push (o->fr, o->mt), from the host record alone
static int online_match_args(const repet_online* o, MatchArgs* a) {
    const repet_online::Frames& fr = o->fr;
    const repet_online::Matches& mt = o->mt;
    repet_ctx* c = o->ctx;
    *a = MatchArgs{};
    if (fr.n <= 0) return REPET_OK;
    a->K = online_max_peaks(o); a->n_frames = fr.n; a->frame0 = fr.first; a->warm = o->M - 1;
    a->slot_start = o->slots_on ? o->slot_start.as<int64_t>() : nullptr;
    if (mt.n_active <= 0) return REPET_OK;
    const int64_t rows = round_up(mt.hist + fr.n, kTile);
    if (fr.S != o->S || mt.n_active > fr.n || mt.idx_pitch < a->K || mt.band_stride < rows * o->LP ||
        c->idx.cap < (size_t)o->S * mt.n_active * mt.idx_pitch * sizeof(int32_t) || c->cnt.cap < (size_t)o->S * mt.n_active * sizeof(int32_t) ||
        o->band.cap < (size_t)o->S * mt.band_stride * sizeof(float))
        return fail(REPET_ERR_LIMIT, "online: the last matches are not in the workspaces");
    a->idx = c->idx.as<int32_t>(); a->cnt = c->cnt.as<int32_t>(); a->band = o->band.as<float>();
    a->idx_stride = mt.n_active * mt.idx_pitch; a->cnt_stride = mt.n_active; a->band_stride = mt.band_stride;
    a->idx_pitch = mt.idx_pitch; a->LP = o->LP; a->lookback = mt.lookback ? 1 : 0;
    a->n_active = mt.n_active; a->hist = mt.hist;
    return REPET_OK;
}

int repet_online_match_capacity(repet_online* o, int32_t* capacity) {
    if (!o || !capacity) return fail(REPET_ERR_BAD_ARG, "null argument");
    *capacity = online_max_peaks(o);
    return REPET_OK;
}

// count int32 [S][n], age int32 and similarity float32 [S][n][K], dense in either form. The host form with no array at all asks for
// the rows; a partly null or short set is refused with the rows still in *n_rows.
static int online_read_matches_impl(repet_online* o, const Reader& r, int64_t* n_rows) {
    if (!o || !n_rows) return fail(REPET_ERR_BAD_ARG, "null argument");
    *n_rows = 0;
    if (!o->fr.valid) return fail(REPET_ERR_BAD_ARG, kStaleMatches);
    const int64_t rows = (int64_t)o->S * o->fr.n, K = online_max_peaks(o);
    *n_rows = rows;
    if (!r.device && (rows == 0 || (!r.part[0] && !r.part[1] && !r.part[2]))) return REPET_OK;
    RP_TRY(read_check(r, rows));
    *n_rows = 0;
    if (rows == 0) return REPET_OK;
    MatchArgs a;
    RP_TRY(online_match_args(o, &a));
    DeviceGuard guard(o->ctx->device);
    const size_t bytes[3] = {(size_t)rows * 4, (size_t)rows * K * 4, (size_t)rows * K * 4};
    void* at[3];
    RP_TRY(read_begin(o, r, bytes, at));
    HIP_TRY(launch_online_matches(a, o->S, static_cast<int32_t*>(at[0]), static_cast<int32_t*>(at[1]), static_cast<float*>(at[2]), o->ctx->stream));
    RP_TRY(read_deliver(o, r, bytes));
    *n_rows = rows;
    return REPET_OK;
}

int repet_online_last_matches(repet_online* o, int32_t* count_out, int32_t* age_out, float* similarity_out, int64_t capacity_rows,
                              int64_t* n_rows) {
    return online_read_matches_impl(o, Reader{false, 3, {count_out, age_out, similarity_out}, capacity_rows, nullptr}, n_rows);
}

int repet_online_last_matches_device(repet_online* o, void* count_dst, void* age_dst, void* similarity_dst, void* signal_stream) {
    int64_t n = 0;
    return online_read_matches_impl(o, Reader{true, 3, {count_dst, age_dst, similarity_dst}, 0, signal_stream}, &n);
}

int repet_online_set_background_gain(repet_online* o, const int32_t* slots, int32_t n_slots, const float* gains) {
    if (!o || !gains) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (slots && n_slots < 0) return fail(REPET_ERR_BAD_ARG, "bad size");
    const int32_t n = slots ? n_slots : 1;
    for (int32_t k = 0; k < n; ++k) {
        if (slots) RP_TRY(check_slot(o, slots[k]));
        RP_TRY(check_background_gain(gains[k]));
    }
    if (n == 0) return REPET_OK;
    repet_ctx* c = o->ctx;
    DeviceGuard guard(c->device);
    if (!slots) {
        HIP_TRY(launch_gain_fill(o->gain_target(), o->S, background_gain_factor(gains[0]), c->stream));
        std::fill(o->gain.begin(), o->gain.end(), gains[0]);
        std::fill(o->gain_dirty.begin(), o->gain_dirty.end(), 1);
        o->n_dirty = o->S;
    } else {
        // a slot named twice takes the last value given for it: the launch gets every slot once
        std::vector<int32_t> ids;
        std::vector<float> a;
        std::vector<unsigned char> seen((size_t)o->S, 0);
        for (int32_t k = 0; k < n; ++k) o->gain[(size_t)slots[k]] = gains[k];
        for (int32_t k = 0; k < n; ++k) {
            const size_t s = (size_t)slots[k];
            if (seen[s]) continue;
            seen[s] = 1;
            ids.push_back(slots[k]);
            a.push_back(background_gain_factor(o->gain[s]));
            if (!o->gain_dirty[s]) { o->gain_dirty[s] = 1; o->n_dirty += 1; }
        }
        HIP_TRY(launch_gain_set(o->gain_target(), ids.data(), a.data(), (int32_t)ids.size(), c->stream));
    }
    o->gains_on = true;
    return REPET_OK;
}

int repet_online_background_gain(repet_online* o, int32_t slot, float* gain_out) {
    if (!o || !gain_out) return fail(REPET_ERR_BAD_ARG, "null argument");
    RP_TRY(check_slot(o, slot));
    *gain_out = o->gain[(size_t)slot];
    return REPET_OK;
}

int repet_online_set_background_band_gains(repet_online* o, const int32_t* slots, int32_t n_slots, const int32_t* edges, int32_t n_bands,
                                           const float* gains, int32_t gains_rows) {
    if (!o || !gains) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (slots && n_slots < 0) return fail(REPET_ERR_BAD_ARG, "bad size");
    const int32_t n = slots ? n_slots : o->S;
    if (gains_rows != 1 && gains_rows != n) return fail(REPET_ERR_BAD_ARG, "online: one row of band gains, or one per slot named");
    if (edges) {
        if (n_bands < 1 || n_bands > o->F) return fail(REPET_ERR_BAD_ARG, "online: between one band and one per bin");
        RP_TRY(check_edges_ascend(o, edges, n_bands));
    } else if (n_bands != o->F) {
        return fail(REPET_ERR_BAD_ARG, "online: without edges there is one gain per bin (window_length / 2 + 1 of them)");
    }
    for (int32_t k = 0; slots && k < n; ++k) RP_TRY(check_slot(o, slots[k]));
    for (int64_t k = 0; k < (int64_t)gains_rows * n_bands; ++k)
        if (!(gains[k] >= 0.f && gains[k] <= 1.f)) return fail(REPET_ERR_BAD_ARG, "online: a band gain lies in [0, 1]");
    if (o->W > 4096) return fail(REPET_ERR_LIMIT, "online: band gains need a window_length of at most 4096");
    if (n == 0) return REPET_OK;
    repet_ctx* c = o->ctx;
    DeviceGuard guard(c->device);
    // a slot named twice takes the last row given for it: the launch gets every slot once. The first set names every slot
    // (row -1: g = 0), and its launch writes the tables' beginning
    const bool init = !o->bands_on;
    std::vector<int32_t> row_of((size_t)o->S, -1);
    for (int32_t k = 0; k < n; ++k) row_of[(size_t)(slots ? slots[k] : k)] = gains_rows == 1 ? 0 : k;
    std::vector<int32_t> ids;
    for (int32_t s = 0; s < o->S; ++s)
        if (init || row_of[(size_t)s] >= 0) ids.push_back(s);
    const int32_t m = (int32_t)ids.size();
    if (init) HIP_TRY(o->band_tab.ensure((size_t)o->S * kBandRows * o->FS * sizeof(float)));
    repet_online::BandJob& job = o->band_job[o->band_job_next];
    if (job.busy) HIP_TRY(hipEventSynchronize(job.done));       // (the launch of kBandJobs sets ago: long over)
    job.busy = false;
    RP_TRY(ensure_pinned(job.p, job.cap, (size_t)band_job_words(m, n_bands, gains_rows) * 4));
    if (!job.done) HIP_TRY(hipEventCreateWithFlags(&job.done, hipEventDisableTiming));
    int32_t* w = static_cast<int32_t*>(job.p);
    for (int32_t i = 0; i < m; ++i) { w[i] = ids[(size_t)i]; w[m + i] = row_of[(size_t)ids[(size_t)i]]; }
    for (int32_t k = 0; k <= n_bands; ++k) w[2 * m + k] = edges ? edges[k] : k;
    std::memcpy(w + 2 * m + n_bands + 1, gains, (size_t)gains_rows * n_bands * sizeof(float));
    HIP_TRY(launch_band_expand(o->band_tab.as<float>(), o->FS, o->F, w, m, n_bands, gains_rows, init, c->stream));
    HIP_TRY(hipEventRecord(job.done, c->stream));
    job.busy = true;
    o->band_job_next = (o->band_job_next + 1) % repet_online::kBandJobs;
    o->bands_on = true;
    for (int32_t s = 0; s < o->S; ++s) {
        const int32_t r = row_of[(size_t)s];
        if (r < 0) continue;
        std::vector<float>& g = o->band_gain[(size_t)s];
        g.assign((size_t)o->F, 0.f);
        bool any = false;
        for (int32_t b = 0; b < n_bands; ++b) {
            const float v = gains[(int64_t)r * n_bands + b];
            const int32_t k0 = edges ? edges[b] : b, k1 = edges ? edges[b + 1] : b + 1;
            for (int32_t k = k0; k < k1; ++k) g[(size_t)k] = v;
            any = any || (v != 0.f && k1 > k0);
        }
        o->band_mark((size_t)s, o->band_stale[(size_t)s] | 1, (unsigned char)((o->band_nd[(size_t)s] & 6) | (any ? 1 : 0)));
    }
    return REPET_OK;
}

int repet_online_background_band_gains(repet_online* o, int32_t slot, float* out, int32_t capacity) {
    if (!o || !out) return fail(REPET_ERR_BAD_ARG, "null argument");
    RP_TRY(check_slot(o, slot));
    if (capacity < o->F) return fail(REPET_ERR_BAD_ARG, "online: output capacity too small (window_length / 2 + 1 values)");
    const std::vector<float>& g = o->band_gain[(size_t)slot];
    for (int32_t k = 0; k < o->F; ++k) out[k] = g.empty() ? 0.f : g[(size_t)k];
    return REPET_OK;
}

int repet_online_set_start_frames(repet_online* o, int32_t start_frames) {
    if (!o) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (o->total_in != 0 || o->epoch != 0 || o->finished) return fail(REPET_ERR_BAD_ARG, "online: start_frames can only be set before the first push");
    if (start_frames < 1 || start_frames > o->B) return fail(REPET_ERR_BAD_ARG, "online: start_frames must lie in [1, buffer_frames]");
    o->M = start_frames;
    return REPET_OK;
}

int repet_online_start_frames(repet_online* o, int32_t* out) {
    if (!o || !out) return fail(REPET_ERR_BAD_ARG, "null argument");
    *out = o->M;
    return REPET_OK;
}

int repet_online_restart_streams(repet_online* o, const int32_t* slots, int32_t n) {
    RP_TRY(online_check_slots(o, slots, n));
    if (o->total_in % o->H) return fail(REPET_ERR_BAD_ARG, "online: a stream can only begin on a hop boundary (samples pushed % step_length == 0)");
    DeviceGuard guard(o->ctx->device);
    return online_reset_slots(o, slots, n, o->total_in / o->H);
}

int repet_online_release_streams(repet_online* o, const int32_t* slots, int32_t n) {
    RP_TRY(online_check_slots(o, slots, n));
    DeviceGuard guard(o->ctx->device);
    return online_reset_slots(o, slots, n, kSlotIdle);
}

static const char* const kHoldGrid = "online: a stream can only be held or resumed on a hop boundary (samples pushed % step_length == 0)";

int repet_online_hold_streams(repet_online* o, const int32_t* slots, int32_t n) {
    RP_TRY(online_check_slots(o, slots, n));
    if (o->total_in % o->H) return fail(REPET_ERR_BAD_ARG, kHoldGrid);
    for (int32_t k = 0; k < n; ++k)
        if (o->start[(size_t)slots[k]] == kSlotIdle) return fail(REPET_ERR_BAD_ARG, "online: the slot is idle");
    DeviceGuard guard(o->ctx->device);
    return online_hold_slots(o, slots, n, true);
}

int repet_online_resume_streams(repet_online* o, const int32_t* slots, int32_t n) {
    RP_TRY(online_check_slots(o, slots, n));
    if (o->total_in % o->H) return fail(REPET_ERR_BAD_ARG, kHoldGrid);
    DeviceGuard guard(o->ctx->device);
    return online_hold_slots(o, slots, n, false);
}

int repet_online_stream_held(repet_online* o, int32_t slot, int32_t* held) {
    if (!o || !held) return fail(REPET_ERR_BAD_ARG, "null argument");
    RP_TRY(check_slot(o, slot));
    *held = o->caller_held[(size_t)slot] ? 1 : 0;
    return REPET_OK;
}

int repet_online_enable_feed(repet_online* o, int64_t capacity_samples) {
    if (!o) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (o->finished) return fail(REPET_ERR_BAD_ARG, "online: stream already finished");
    if (o->feed_cap > 0) return fail(REPET_ERR_BAD_ARG, "online: the handle has its inboxes already (enable_feed is made once)");
    if (capacity_samples < o->H) return fail(REPET_ERR_BAD_ARG, "online: an inbox holds at least one hop (capacity_samples >= step_length)");
    if (capacity_samples * (int64_t)o->C > INT32_MAX) return fail(REPET_ERR_LIMIT, "online: an inbox holds fewer than 2^31 values");
    if (o->total_in % o->H) return fail(REPET_ERR_BAD_ARG, "online: the inboxes can only be enabled on a hop boundary (samples pushed % step_length == 0)");
    repet_ctx* c = o->ctx;
    DeviceGuard guard(c->device);
    const int64_t stride = round_up(capacity_samples * o->C, 4);
    HIP_TRY(o->ring.ensure((size_t)2 * o->S * stride * sizeof(float)));
    HIP_TRY(hipMemsetAsync(o->ring.p, 0, (size_t)2 * o->S * stride * sizeof(float), c->stream));
    RP_TRY(ensure_io_events(c));
    o->ring_stride = stride;
    o->q_count.assign((size_t)o->S, 0);
    o->q_read.assign((size_t)o->S, 0);
    o->feed_cap = capacity_samples;
    return REPET_OK;
}

int repet_online_feed(repet_online* o, const int32_t* slots, const int64_t* counts, int32_t n_slots, const void* audio, int dtype, int64_t n) {
    FeedPlan plan;
    RP_TRY(online_feed_plan(o, slots, counts, n_slots, n, &plan));
    if (dtype < REPET_F32 || dtype > REPET_I16) return fail(REPET_ERR_BAD_ARG, "bad size or dtype");
    if (n_slots == 0 || n == 0) return REPET_OK;
    if (!audio) return fail(REPET_ERR_BAD_ARG, "null argument");
    repet_ctx* c = o->ctx;
    DeviceGuard guard(c->device);
    // the rows [n_slots][n][C] through the pinned buffer into the staging buffer, then into the rings on the device
    const size_t esz = dtype == REPET_F64 ? 8 : (dtype == REPET_F32 ? 4 : 2);
    RP_TRY(online_upload(o, audio, (size_t)n_slots * n * o->C * esz));
    const int64_t dense[3] = {n * o->C, o->C, 1};
    return online_feed_launch(o, plan, o->staging.p, dtype, n, dense);
}

int repet_online_feed_device(repet_online* o, const int32_t* slots, const int64_t* counts, int32_t n_slots, const void* src, int dtype,
                             int64_t n, const int64_t src_strides[3], void* wait_stream, void* signal_stream) {
    FeedPlan plan;
    RP_TRY(online_feed_plan(o, slots, counts, n_slots, n, &plan));
    if (dtype < REPET_F32 || dtype > REPET_BF16) return fail(REPET_ERR_BAD_ARG, "bad size or dtype");
    RP_TRY(check_strides(src_strides));
    if (n_slots == 0 || n == 0) return REPET_OK;
    if (!src) return fail(REPET_ERR_BAD_ARG, "null argument");
    repet_ctx* c = o->ctx;
    DeviceGuard guard(c->device);
    RP_TRY(wait_caller(c, wait_stream, signal_stream));
    RP_TRY(online_feed_launch(o, plan, src, dtype, n, src_strides));
    // the caller's stream continues behind the copy: the packet may be overwritten once that stream gets there
    return signal_caller(c, signal_stream);
}

int repet_online_queued(repet_online* o, int32_t slot, int64_t* queued) {
    if (!o || !queued) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (o->feed_cap <= 0) return fail(REPET_ERR_BAD_ARG, kNoFeed);
    if (slot >= 0) {
        RP_TRY(check_slot(o, slot));
        *queued = o->q_count[(size_t)slot];
        return REPET_OK;
    }
    for (size_t s = 0; s < (size_t)o->S; ++s) queued[s] = o->q_count[s];
    return REPET_OK;
}

int repet_online_pad_feed(repet_online* o, const int32_t* slots, int32_t n_slots, int64_t* pads) {
    RP_TRY(online_check_feed(o));
    if (!pads || (slots && n_slots < 0)) return fail(REPET_ERR_BAD_ARG, "null argument");
    // every live slot where none is named (an idle one pads nothing); named, an idle slot is refused as feed refuses it
    std::vector<int32_t> ids;
    if (slots) ids.assign(slots, slots + n_slots);
    else for (int32_t s = 0; s < o->S; ++s) if (o->start[(size_t)s] != kSlotIdle) ids.push_back(s);
    std::vector<int64_t> counts;
    for (int32_t s : ids) {
        RP_TRY(check_slot(o, s));
        counts.push_back((o->H - o->q_count[(size_t)s] % o->H) % o->H);
    }
    FeedPlan plan;
    RP_TRY(online_feed_plan(o, ids.data(), counts.data(), (int32_t)ids.size(), o->H, &plan));
    repet_ctx* c = o->ctx;
    DeviceGuard guard(c->device);
    bool any = false;
    for (int64_t cnt : counts) any = any || cnt > 0;
    if (any) {
        // one hop of zeros that every row reads (row stride 0)
        const size_t bytes = (size_t)o->H * o->C * sizeof(float);
        HIP_TRY(o->staging.ensure(bytes));
        HIP_TRY(hipMemsetAsync(o->staging.p, 0, bytes, c->stream));
        const int64_t strides[3] = {0, o->C, 1};
        RP_TRY(online_feed_launch(o, plan, o->staging.p, REPET_F32, o->H, strides));
    }
    if (slots) for (size_t k = 0; k < ids.size(); ++k) pads[k] = counts[k];
    else {
        for (int32_t s = 0; s < o->S; ++s) pads[s] = 0;
        for (size_t k = 0; k < ids.size(); ++k) pads[(size_t)ids[k]] = counts[k];
    }
    return REPET_OK;
}

int repet_online_clear_feed(repet_online* o, const int32_t* slots, int32_t n_slots) {
    if (!o) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (o->feed_cap <= 0) return fail(REPET_ERR_BAD_ARG, kNoFeed);
    if (slots && n_slots < 0) return fail(REPET_ERR_BAD_ARG, "bad size");
    for (int32_t k = 0; slots && k < n_slots; ++k) RP_TRY(check_slot(o, slots[k]));
    // host counters alone: the launches that filled the rings stay where they are in the stream, and what they wrote is
    // overwritten by the feeds that follow before any take reads it
    if (!slots) { std::fill(o->q_count.begin(), o->q_count.end(), 0); std::fill(o->q_read.begin(), o->q_read.end(), 0); }
    else for (int32_t k = 0; k < n_slots; ++k) { o->q_count[(size_t)slots[k]] = 0; o->q_read[(size_t)slots[k]] = 0; }
    return REPET_OK;
}

int repet_online_tick(repet_online* o, int64_t hops, double* out, int64_t capacity, uint8_t* consumed, int64_t* n_written) {
    AlsoScope also(o);
    return online_tick_impl(o, hops, host_sink(out, capacity), consumed, n_written);
}

int repet_online_tick_device(repet_online* o, int64_t hops, void* dst, int dst_dtype, const int64_t dst_strides[3], void* signal_stream,
                             uint8_t* consumed, int64_t* n_written) {
    AlsoScope also(o);
    return online_tick_impl(o, hops, device_sink(dst, dst_dtype, dst_strides, signal_stream), consumed, n_written);
}

int repet_online_stream_emit_count(repet_online* o, int32_t slot, int64_t* n_emit) {
    int64_t n_new = 0;
    return online_plan_slot(o, slot, &n_new, n_emit);
}

int repet_online_finish_stream(repet_online* o, int32_t slot, double* out, int64_t capacity, int64_t* n_written) {
    AlsoScope also(o);
    return online_finish_stream_impl(o, slot, host_sink(out, capacity), n_written);
}

int repet_online_finish_stream_device(repet_online* o, int32_t slot, void* dst, int dst_dtype, const int64_t dst_strides[2],
                                      void* signal_stream, int64_t* n_written) {
    AlsoScope also(o);
    if (!dst_strides) return fail(REPET_ERR_BAD_ARG, "null argument");
    const int64_t strides[3] = {0, dst_strides[0], dst_strides[1]};        // (the ABI takes the two strides of [n][C])
    return online_finish_stream_impl(o, slot, device_sink(dst, dst_dtype, strides, signal_stream), n_written);
}

int repet_online_stream_state_size(repet_online* o, int64_t* header_bytes, int64_t* payload_bytes) {
    if (!o || !header_bytes || !payload_bytes) return fail(REPET_ERR_BAD_ARG, "null argument");
    *header_bytes = (int64_t)sizeof(StateHeader);
    *payload_bytes = state_layout(o).floats * (int64_t)sizeof(float);
    return REPET_OK;
}

// the 4-byte alignment refusal is the device form's alone; the header goes out once the payload's launch is enqueued (device) or
// has been waited for (host)
static int online_read_export_impl(repet_online* o, int32_t slot, void* header_out, const Reader& r) {
    if (!o || !header_out || !r.part[0]) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (r.device && (reinterpret_cast<uintptr_t>(r.part[0]) & 3)) return fail(REPET_ERR_BAD_ARG, "online: the payload must be 4-byte aligned");
    StateHeader h;
    RP_TRY(online_export_plan(o, slot, &h));
    DeviceGuard guard(o->ctx->device);
    const size_t bytes = (size_t)h.payload_bytes;
    void* at = nullptr;
    RP_TRY(read_begin(o, r, &bytes, &at));
    RP_TRY(online_export(o, slot, h, static_cast<float*>(at)));
    RP_TRY(read_deliver(o, r, &bytes));
    std::memcpy(header_out, &h, sizeof(h));
    return REPET_OK;
}

int repet_online_export_stream(repet_online* o, int32_t slot, void* header_out, void* payload_out) {
    return online_read_export_impl(o, slot, header_out, host_reader(payload_out, 0));
}

int repet_online_export_stream_device(repet_online* o, int32_t slot, void* header_out, void* payload_dev, void* signal_stream) {
    return online_read_export_impl(o, slot, header_out, device_reader(payload_dev, signal_stream));
}

// The data flows the other way: r.part[0] is read, through the pinned buffer (host) or where it lies behind the caller's stream
// (device), which then continues behind the import: the payload may be reused once that stream gets there.
static int online_import_impl(repet_online* o, int32_t slot, const void* header, const Reader& r) {
    if (!o || !header || !r.part[0]) return fail(REPET_ERR_BAD_ARG, "null argument");
    if (r.device && (reinterpret_cast<uintptr_t>(r.part[0]) & 3)) return fail(REPET_ERR_BAD_ARG, "online: the payload must be 4-byte aligned");
    StateHeader h;
    std::memcpy(&h, header, sizeof(h));
    RP_TRY(online_import_check(o, slot, &h));
    DeviceGuard guard(o->ctx->device);
    if (r.device) RP_TRY(wait_caller(o->ctx, r.stream, r.stream));
    else RP_TRY(online_upload(o, r.part[0], (size_t)h.payload_bytes));
    RP_TRY(online_import(o, slot, h, static_cast<const float*>(r.device ? r.part[0] : o->staging.p)));
    return r.device ? signal_caller(o->ctx, r.stream) : REPET_OK;
}

int repet_online_import_stream(repet_online* o, int32_t slot, const void* header, const void* payload) {
    return online_import_impl(o, slot, header, host_reader(const_cast<void*>(payload), 0));
}

int repet_online_import_stream_device(repet_online* o, int32_t slot, const void* header, const void* payload_dev, void* wait_stream) {
    return online_import_impl(o, slot, header, device_reader(const_cast<void*>(payload_dev), wait_stream));
}

int repet_online_open_streams(int device, int32_t n_streams, int32_t n_channels, const repet_params* p, int64_t max_push_samples,
                              repet_online** out) {
    if (!out) return fail(REPET_ERR_BAD_ARG, "out is null");
    if (n_streams < 1 || n_streams > 65535) return fail(REPET_ERR_BAD_ARG, "online: between 1 and 65535 streams");
    if (n_channels < 1) return fail(REPET_ERR_BAD_ARG, "online: at least one channel");
    if (max_push_samples < 0) return fail(REPET_ERR_BAD_ARG, "online: negative max_push_samples");
    RP_TRY(check_params(p));
    if (p->buffer_frames < 2 || p->sim_number < 1) return fail(REPET_ERR_BAD_ARG, "online: bad buffer length or similarity number");
    auto* o = new repet_online();
    int rc = repet_ctx_create(device, &o->ctx);
    if (rc != REPET_OK) { delete o; return rc; }
    o->p = *p; o->S = n_streams; o->C = n_channels; o->W = p->window_length; o->H = p->step_length; o->F = o->W / 2 + 1;
    o->FS = (int)round_up(o->F, kFreqAlign); o->B = p->buffer_frames; o->M = o->B; o->Hh = o->B - 1; o->LP = (int)round_up(o->B, 64);
    o->max_push = max_push_samples;
    o->start.assign((size_t)n_streams, 0);
    o->held.assign((size_t)n_streams, 0);
    o->caller_held.assign((size_t)n_streams, 0);
    o->starved.assign((size_t)n_streams, 0);
    o->band_gain.assign((size_t)n_streams, std::vector<float>());
    o->band_stale.assign((size_t)n_streams, 0);
    o->band_nd.assign((size_t)n_streams, 0);
    {   // every slot's stream begins with the handle's until a restart or release says otherwise
        DeviceGuard guard(o->ctx->device);
        hipError_t e = o->slot_start.ensure((size_t)n_streams * sizeof(int64_t));
        if (e == hipSuccess) e = hipMemsetAsync(o->slot_start.p, 0, (size_t)n_streams * sizeof(int64_t), o->ctx->stream);
        // the background gains: 0 for every slot, which is a = 1 in the target table and in both current ones
        o->gain.assign((size_t)n_streams, 0.f);
        o->gain_dirty.assign((size_t)n_streams, 0);
        if (e == hipSuccess) e = o->gain_tab.ensure((size_t)3 * n_streams * sizeof(float));
        if (e == hipSuccess) e = launch_gain_fill(o->gain_tab.as<float>(), 3 * n_streams, 1.f, o->ctx->stream);
        if (e != hipSuccess) { repet_online_close(o); return fail(e == hipErrorOutOfMemory ? REPET_ERR_OOM : REPET_ERR_HIP, hipGetErrorString(e)); }
    }
    if (max_push_samples > 0) {
        // a push of up to max_push_samples completes at most max_push / H + 1 frames, the finish at most W / H + 1
        DeviceGuard guard(o->ctx->device);
        const int64_t frames = std::max<int64_t>(max_push_samples / o->H + 1, o->W / o->H + 1);
        rc = online_ensure_windows(o, frames);
        if (rc == REPET_OK) rc = online_ensure_pending(o, max_push_samples + o->W);
        if (rc == REPET_OK) rc = ensure_io_events(o->ctx);
        if (rc != REPET_OK) { repet_online_close(o); return rc; }
    }
    *out = o;
    return REPET_OK;
}

int repet_online_open(int device, int32_t n_channels, const repet_params* p, repet_online** out) {
    return repet_online_open_streams(device, 1, n_channels, p, 0, out);
}

int repet_online_close(repet_online* o) {
    if (!o) return REPET_OK;
    {
        DeviceGuard guard(o->ctx->device);
        (void)hipStreamSynchronize(o->ctx->stream);
        for (int k = 0; k < 2; ++k) { o->X[k].release(); o->V[k].release(); o->Vn[k].release(); o->pend[k].release(); o->pend_lo[k].release(); }
        o->band_tab.release(); o->outs.release();
        for (auto& j : o->band_job) {
            free_pinned(j.p, j.cap);
            if (j.done) (void)hipEventDestroy(j.done);
            j.done = nullptr;
        }
        o->band.release(); o->outf.release(); o->out64.release(); o->staging.release(); o->slot_start.release(); o->gain_tab.release(); o->levels.release(); o->ring.release();
        free_pinned(o->host_in, o->host_in_cap);
        free_pinned(o->host_out, o->host_out_cap);
    }
    repet_ctx_destroy(o->ctx);
    delete o;
    return REPET_OK;
}

int repet_online_emit_count(repet_online* o, int64_t n, int finishing, int64_t* n_emit) {
    if (!o || !n_emit) return fail(REPET_ERR_BAD_ARG, "null argument");
    int64_t n_new = 0;
    return online_plan(o, n, finishing != 0, &n_new, n_emit);
}

int repet_online_push_streams(repet_online* o, const void* audio, int dtype, int64_t n, double* out, int64_t capacity,
                              int64_t* n_written) {
    AlsoScope also(o);
    return online_push_impl(o, audio, dtype, n, nullptr, nullptr, host_sink(out, capacity), n_written);
}

int repet_online_push(repet_online* o, const void* audio, int dtype, int64_t n, double* out, int64_t capacity,
                      int64_t* n_written) {
    return repet_online_push_streams(o, audio, dtype, n, out, capacity, n_written);
}

int repet_online_push_device(repet_online* o, const void* src, int dtype, int64_t n, const int64_t src_strides[3],
                             void* wait_stream, void* dst, int dst_dtype, const int64_t dst_strides[3], void* signal_stream,
                             int64_t* n_written) {
    AlsoScope also(o);
    return online_push_impl(o, src, dtype, n, src_strides, wait_stream, device_sink(dst, dst_dtype, dst_strides, signal_stream), n_written);
}

int repet_online_finish_streams(repet_online* o, double* out, int64_t capacity, int64_t* n_written) {
    AlsoScope also(o);
    return online_finish_impl(o, host_sink(out, capacity), n_written);
}

int repet_online_finish(repet_online* o, double* out, int64_t capacity, int64_t* n_written) {
    return repet_online_finish_streams(o, out, capacity, n_written);
}

int repet_online_finish_device(repet_online* o, void* dst, int dst_dtype, const int64_t dst_strides[3], void* signal_stream,
                               int64_t* n_written) {
    AlsoScope also(o);
    return online_finish_impl(o, device_sink(dst, dst_dtype, dst_strides, signal_stream), n_written);
}

}  // extern "C"
