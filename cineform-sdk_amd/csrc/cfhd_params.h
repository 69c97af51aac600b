// cfhd_params.h -- what CFHD_PrepareToEncode derives from its arguments, for the other front ends of the same encoder (cfhd_batch.cpp).
#pragma once
#include "cfhd_core.h"
#include "cfhd_gop.h"
#include <stdint.h>

namespace cfhd {

struct FrontEndParams {
	int pixel_kind = 0, encoded_format = 0, pixel_bytes = 2;
	int color_format = 2, color_space = 2, quality = 0;      // as the sample header carries them (quality incl. the 4:4:4:4 marker)
	bool progressive = true;
	bool static_quantizer = true;                             // false: the quality re-derives its tables from the size of the previous sample (rate feedback)
	FramePlan plan;                                           // geometry + first-frame quantizer
	// what the rate feedback goes on from (cfhd_batch.cpp, the frame queue's streams): the quality word derive_quantization takes -- the caller's with the format
	// marks, where `quality` above is the header's -- and the quantizer state behind the derivation of the first frame's tables
	int derive_quality = 0; QuantState qstate = {0, -1, 0};
	// CFHD_ENCODING_FLAGS_YUV_2FRAME_GOP: the group's plan with its quantizer tables; whether those tables follow the size of the previous key sample (rate feedback);
	// whether the input's own pixel format is an output a group of this scan and width decodes to at full resolution; the input format of the sequence header
	bool gop = false, gop_static_quantizer = true, gop_output_served = false;
	int gop_sequence_format = 0;
	GopPlan gplan; QuantState gqstate = {0, -1, 0};           // (the group encoder's state behind CFHD_PrepareToEncode: what a group stream's walk starts from)
};
// Same checks and derivations as CFHD_PrepareToEncode (cfhd_api.cpp make_params).  Returns a CFHD_Error value (0 = OK).
int front_end_params(int width, int height, uint32_t pixel_format, int encoded_format, uint32_t encoding_flags, int quality, FrontEndParams *out);
// What a decoder handle knows once CFHD_PrepareToDecode has accepted a whole sample, for the other front end of the same decoder (the decode queue,
// cfhd_decode_queue.hip): the handle's own gates decide, this only reads their result.  Returns 0, or -1 for a handle that is not prepared on an intra sample.
struct DecoderHandleState {
	FramePlan plan;                                           // geometry, precision, prescale, colour matrix: as the handle decodes every sample it is given
	int out_kind = 0, encoded_format = 0, color_space = 0;
	bool half = false, interlaced = false, progressive_flag = false;      // of the sample the handle was prepared on (the whole sample: the flag lies behind the first 512 bytes)
	size_t sample_cap = 0;                                    // the longest sample the handle's device stage takes
};
int decoder_handle_state(void *decoder_ref, DecoderHandleState *out);
// The same for a handle prepared on a stream of two-frame groups that has decoded its first group (the scan is known from there): 0, or -1 for any other handle.
struct DecoderGroupState {
	GopPlan plan;                                             // geometry and scan, as the handle decodes every group it is given
	int out_kind = 0;
	bool half = false;
};
int decoder_group_state(void *decoder_ref, DecoderGroupState *out);
// Forgets the group the handle decoded last: the P-frame sample it is given next has no picture to hand out (the state of a freshly prepared handle).
void decoder_group_reset(void *decoder_ref);

} // namespace cfhd
