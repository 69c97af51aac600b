// group_stream_hooks.cpp -- TEST-ONLY C entry of tests/group_stream_batches.py: the divisors a group sample's band headers carry (the product's host parser,
// cfhd_gop.cpp parse_group_sample).  Built by the helper from this file and the product's host-only sources; not part of libcfhd_amd.so.
#include "cfhd_core.h"
#include "cfhd_bitstream.h"
#include "cfhd_gop.h"

using namespace cfhd;

extern "C" {

// Per channel: the wavelets in the order the sample codes them (w[5], w[4], w[3], w[1], w[0]), bands 1 .. 3 of each and band 0 of w[3] in front of its others --
// 16 divisors a channel.  Returns the count, or < 0 for a sample the parser refuses or one without a coded band where the group syntax has one.
int cfhd_amd_group_sample_quants(const uint8_t *sample, size_t size, int *out)
{
	ParsedGroup pg;
	if (parse_group_sample(sample, size, &pg) != 0) return -1;
	static const int coded[5] = { 5, 4, 3, 1, 0 };
	int n = 0;
	for (int c = 0; c < 3; c++)
		for (int k : coded)
			for (int b = (k == 3 ? 0 : 1); b < 4; b++) {
				if (!pg.band[c][k][b].present) return -2;
				out[n++] = pg.band[c][k][b].quant;
			}
	return n;
}

}
