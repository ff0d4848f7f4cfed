// The similar frames a streaming handle matched (repet_online_last_matches*): for every frame the last push completed and
// every slot, the list the mask's median was taken over (repet.py:861-866), read where the push left it. The peak picking wrote
// the lists into idx / cnt as rows of the push's window, counted from the window's first valid row; the frame itself is a row of
// that window too, and a slot's window holds its own frames only, one per row, so
//   age        = the frame's row - the entry: 0 the frame itself, 1 the frame before, in the slot's own frames
//   similarity = the fp32 entry of the band the peak picking read: band[row][age] in the look-back layout (band[j][l] =
//                sim(j, j - l)), band[entry][age] in the diagonal one (band[t][l] = sim(t, t + l), REPET_GRAM=f32)
// The order inside idx is the engine's; the output is ordered by age. Ages are distinct, so an entry's place is the number of
// entries with a larger row (equal rows, which the peak picking never writes, would fall in list order: every place below
// count is written exactly once whatever idx holds). One wavefront per (frame, slot): a lane owns entry 64 q + lane, the
// others' rows come round by __shfl, 64 at a time; lists longer than 64 take further rounds. No LDS, no atomics: the same bits
// from every call.
// Which rows have a list is decided as the mask kernel decides it (mask.hip: warm_up_end), from the slot table the push's own
// kernels read: a frame before its slot's own frame start_frames - 1 (an idle or held slot: every frame) has none, and cnt is
// not read there -- the peak picking does not write it for every such row. Every bound comes from the host's record of the
// push; an entry outside [0, row] or a lag past the band's pitch, which the peak picking never writes, is not followed into
// the band (similarity 0).
#include "engine.h"

namespace repet_eng {
namespace {

__global__ __launch_bounds__(64) void online_matches_kernel(MatchArgs a, int32_t* __restrict__ count, int32_t* __restrict__ age,
                                                           float* __restrict__ similarity) {
    const int slot = blockIdx.y, lane = threadIdx.x;
    const int64_t t = blockIdx.x;
    const int64_t out = slot * a.n_frames + t;
    int32_t* age_row = age + out * a.K;
    float* sim_row = similarity + out * a.K;
    const int64_t start = a.slot_start ? a.slot_start[slot] : 0;      // kSlotIdle / kSlotHeld: past every frame
    const int64_t r = t - (a.n_frames - a.n_active);                   // the frame's list row (handle warm-up frames have none)
    int n = 0;
    if (r >= 0 && a.frame0 + t - start >= a.warm) n = min(max(a.cnt[slot * a.cnt_stride + r], 0), a.K);
    n = __builtin_amdgcn_readfirstlane(n);                             // (uniform: one row per wavefront)
    const int32_t* list = a.idx + slot * a.idx_stride + r * a.idx_pitch;
    const float* band = a.band + slot * a.band_stride;
    const int64_t row = a.hist + t;                                    // the frame's own window row
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        const bool mine = k < n;
        const int e = mine ? list[k] : 0;
        int place = 0;
        for (int c0 = 0; c0 < n; c0 += 64) {
            const int other = c0 + lane < n ? list[c0 + lane] : 0;
            const int m = min(64, n - c0);
            for (int l = 0; l < m; ++l) {
                const int v = __shfl(other, l);
                place += (v > e || (v == e && c0 + l < k)) ? 1 : 0;
            }
        }
        if (mine) {
            const int64_t lag = row - e;
            const bool inside = e >= 0 && lag >= 0 && lag < a.LP;
            age_row[place] = (int32_t)lag;
            sim_row[place] = inside ? band[(a.lookback ? row : (int64_t)e) * a.LP + lag] : 0.f;
        }
    }
    for (int k = n + lane; k < a.K; k += 64) {
        age_row[k] = -1;
        sim_row[k] = 0.f;
    }
    if (lane == 0) count[out] = n;
}

}  // namespace

hipError_t launch_online_matches(const MatchArgs& a, int32_t n_streams, int32_t* count, int32_t* age, float* similarity, hipStream_t s) {
    if (n_streams <= 0 || a.n_frames <= 0) return hipSuccess;
    if (!count || !age || !similarity || a.K < 1 || n_streams > 65535 || a.n_frames > 0x7fffffff || a.n_active < 0 || a.n_active > a.n_frames ||
        a.hist < 0 || (a.n_active > 0 && (!a.idx || !a.cnt || !a.band || a.idx_pitch < a.K || a.LP < 1)))
        return hipErrorInvalidValue;
    online_matches_kernel<<<dim3((unsigned)a.n_frames, (unsigned)n_streams), 64, 0, s>>>(a, count, age, similarity);
    return hipGetLastError();
}

}  // namespace repet_eng
