// The two FFT launchers with the kernel family as an ARGUMENT and a report of what they launched (stage tests:
// repet_debug_stft_stage / repet_debug_istft_stage, engine_stages.hip). REPET_FFT_PATH is read once per process, so one
// process sees one family through launch_stft(a, s) / launch_istft_ola(a, s); those stay the "as production picks" form
// and are the path = kFftPathAuto case of the functions below -- same conditions, same kernels, same launch geometry.
#pragma once
#include "common.h"

namespace repet {

enum FftPath { kFftPathAuto = 0, kFftPathBlock = 1, kFftPathWave = 2, kFftPathReg = 3 };

// family: kFftPathBlock / Wave / Reg of the kernel launched, 0 when nothing was launched (no frames, no samples)
// run: frames (forward) or hops (inverse) per workgroup as the launcher chose them; the register kernels: forward 12 frames
//      per workgroup and round, inverse 12 R - 1 hops (`run`) from R rounds (`rounds`)
// slots: resident workgroups of the device the run was fitted to (block kernels), the CU count (register kernels)
// launches: kernel launches made (> 1: the channel groups of launch_istft_ola; `kernel` etc. describe the last one)
struct FftLaunch {
    const char* kernel = "";
    int family = 0, run = 0, rounds = 0, slots = 0, launches = 0;
    int64_t workgroups = 0, units = 0;
};

// A family asked for by name that does not take the shape (reg: W != 2048, inverse with more than two channels; wave:
// W = 8192, forward with more than eight channels, inverse with three or more than four) is hipErrorInvalidValue -- the
// launchers' answer to arguments they cannot serve -- never another family's kernel.
bool reg_fft_supported(int W, int n_channels, bool inverse, int path);
hipError_t launch_stft(const StftArgs& a, hipStream_t s, int path, FftLaunch* info);
hipError_t launch_istft_ola(const IstftOlaArgs& a, hipStream_t s, int path, FftLaunch* info);
hipError_t launch_stft_reg(const StftArgs& a, hipStream_t s, FftLaunch* info);
hipError_t launch_istft_ola_reg(const IstftOlaArgs& a, int64_t hops, hipStream_t s, FftLaunch* info);

}  // namespace repet
