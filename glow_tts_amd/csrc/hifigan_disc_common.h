// The limits and the argument checks of the HiFi-GAN multi-period discriminator, shared by its f32 launches (hifigan_disc_ops.hip) and its bf16 mode
// (hifigan_disc_bf16_ops.hip).  Host side alone: the row map `hd_source_row` is hifigan_common.h's.
#pragma once
#include "hifigan_common.h"

namespace {

constexpr int HD_TAPS = 5, HD_POST_TAPS = 3, HD_MAX_PERIOD = 16, HD_MAX_CHANNELS = 1024;

bool hd_period(int p) { return p >= 2 && p <= HD_MAX_PERIOD; }
bool hd_width(int C) { return C >= 16 && C <= HD_MAX_CHANNELS && C % 16 == 0; }
bool hd_stride(int s) { return s == 1 || s == 3; }
int hd_rows_out(int H, int s) { return (H - 1) / s + 1; }
// every batch row of the full length: B H p <= 2^30 rows (a grid of one thread per row and four channels stays below 2^31 workgroups at 1024 channels)
bool hd_bad_rows(int B, int H, int p) { return B < 1 || B > 65535 || H < 1 || !hd_period(p) || (int64_t)B * H * p > ((int64_t)1 << 30); }

}  // namespace
