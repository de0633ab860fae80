// knn_wide.hpp -- host-only arithmetic of the wide fp16 filter scan (k_scan_f16_qsw, knn_bf16.hip): the column pitch of the
// 16-bit copies and the register home of a stationary query fragment.  No HIP in here: tests/test_knn_wide_host.py compiles it
// with the host compiler and checks it against values written out by hand.
#pragma once

constexpr int LEMON_QSW_MAX_D = 1280;          // widest embedding the register-resident scans serve (ViT-bigG/14)

// Column pitch of the 16-bit copies of Q and X.  The Q-stationary kernels are instantiated per pitch: 256 / 512 / 768
// (k_scan_bf16_qs, _qs2, k_scan_f16_qs4) and, with the wide filter switched on (lemon_index_set_wide_filter), 1024 / 1280
// (k_scan_f16_qsw).  Every other width is streamed by k_scan_bf16 at the next multiple of its 64-wide k-slice.
inline int lemon_bf16_pitch(int d, bool wide) {
    if (d <= 256) return 256;
    if (d <= 512) return 512;
    if (d <= 768) return 768;
    if (wide && d <= 1024) return 1024;
    if (wide && d <= LEMON_QSW_MAX_D) return 1280;
    return (d + 63) / 64 * 64;
}

// k_scan_f16_qsw keeps 2 query groups x NS = pitch / 32 k32 steps of fragments (four registers each) per wave.
// Fragment (group b, step s) has index f = b NS + s; the first 64 live in the 256 AccVGPRs, the rest in VGPRs.
constexpr int LEMON_QSW_ACC_FRAGS = 64;
inline int lemon_qsw_steps(int pitch) { return pitch / 32; }
inline int lemon_qsw_frag_index(int pitch, int b, int s) { return b * lemon_qsw_steps(pitch) + s; }
inline bool lemon_qsw_frag_in_acc(int pitch, int b, int s) { return lemon_qsw_frag_index(pitch, b, s) < LEMON_QSW_ACC_FRAGS; }
// registers a wave holds for the scan: (AccVGPRs, VGPRs for fragments, VGPRs for the 4 x 2 accumulator tiles)
inline void lemon_qsw_register_homes(int pitch, int *acc_regs, int *vgpr_frag_regs, int *vgpr_tile_regs) {
    const int frags = 2 * lemon_qsw_steps(pitch);
    const int in_acc = frags < LEMON_QSW_ACC_FRAGS ? frags : LEMON_QSW_ACC_FRAGS;
    *acc_regs = 4 * in_acc;
    *vgpr_frag_regs = 4 * (frags - in_acc);
    *vgpr_tile_regs = 4 * 2 * 4;
}
