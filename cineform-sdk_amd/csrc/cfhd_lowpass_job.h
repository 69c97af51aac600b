// cfhd_lowpass_job.h -- the record the sample parsers (k_dec_parse, k_dec_parse_group: cfhd_entropy_kernels.h) and the host's job builders write per sample and channel
// for the raw lowpass band: where its big-endian 16-bit words lie inside the sample, and where k_dec_lowpass puts them.  A header of its own because two kernel
// headers that never meet in one translation unit read it: cfhd_entropy_kernels.h (k_dec_lowpass) and cfhd_thumbnail_kernels.h (k_dec_thumbnail).
#pragma once
#include <stdint.h>

namespace cfhd {
namespace dev {

// src: width x height words, rows back to back (null or width 0: no band); dst, pitch, bias: the band raster of the coefficient pyramid and what is added on the way
struct DecLowpassJob { const uint8_t *src; int16_t *dst; int width, height, pitch, bias; };

} // namespace dev
} // namespace cfhd
