// tests/gpu_prims/prims.hip -- TEST INFRASTRUCTURE ONLY: one C entry per primitive of <cfhd_gfx950.h>, each a tiny kernel over caller-supplied arrays.
// Built twice from this one source (tests/test_gpu_primitives.py): by hipcc for gfx950 over cineform-sdk_amd/csrc (the real header: DPP, v_pk_*, v_perm,
// inline asm) and by g++ over tests/hipemu (the scalar twin, launches rewritten by translate_launches.py).  Never part of libcfhd_amd.so.
#include <stdint.h>
#include <hip/hip_runtime.h>
#include <cfhd_gfx950.h>

using namespace cfhd::dev;

enum { OP_ADDS, OP_SUBS, OP_ADDW, OP_NEGW, OP_MAXS, OP_SRA, OP_MULW, OP_LOLO, OP_HIHI, OP_TO8, OP_TO8_BYTES, OP_PERM, OP_ROTR, OP_MUL24, OP_LDG32, OP_LDG64, OP_LDG128 };

// out[i] = op(a[i], b[i], c[i], d[i]); s: the wave-uniform shift of pk_sra / pk_to8 / pk_to8_bytes (a kernel argument, as in the product's kernels)
template <int OP> __global__ void __launch_bounds__(256) k_map(const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *out, int n, int s)
{
	for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x)) {
		uint32_t r = 0;
		if (OP == OP_ADDS) r = pk_adds(a[i], b[i]);
		if (OP == OP_SUBS) r = pk_subs(a[i], b[i]);
		if (OP == OP_ADDW) r = pk_addw(a[i], b[i]);
		if (OP == OP_NEGW) r = pk_negw(a[i]);
		if (OP == OP_MAXS) r = pk_maxs(a[i], b[i]);
		if (OP == OP_SRA) r = pk_sra(a[i], s);
		if (OP == OP_MULW) r = pk_mulw(a[i], b[i]);
		if (OP == OP_LOLO) r = pk_lolo(a[i], b[i]);
		if (OP == OP_HIHI) r = pk_hihi(a[i], b[i]);
		if (OP == OP_TO8) r = pk_to8(a[i], s, c[i]);
		if (OP == OP_TO8_BYTES) r = pk_to8_bytes(a[i], b[i], s, c[i], d[i]);
		if (OP == OP_PERM) r = byte_perm(a[i], b[i], c[i]);
		if (OP == OP_ROTR) r = rotr32(a[i], b[i]);
		if (OP == OP_MUL24) r = mul_u24(a[i], b[i]);
		if (OP == OP_LDG32) r = CFHD_LDG32(a + i);
		if (OP == OP_LDG64) { const cfhd_u2 v = CFHD_LDG64(a + 2 * (i >> 1)); r = (i & 1) ? v.y : v.x; }
		if (OP == OP_LDG128) { const cfhd_u4 v = CFHD_LDG128(a + 4 * (i >> 2)); r = (i & 3) == 0 ? v.x : ((i & 3) == 1 ? v.y : ((i & 3) == 2 ? v.z : v.w)); }
		out[i] = r;
	}
}

// whole waves only (n a multiple of the workgroup size): scan[i] = wave_incl_scan(x[i]); mbcnt[i] = wave_mbcnt(ballot of pred[i] != 0)
__global__ void __launch_bounds__(256) k_wave(const uint32_t *x, const uint32_t *pred, uint32_t *scan, uint32_t *mbcnt)
{
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	scan[i] = wave_incl_scan(x[i]);
	const unsigned long long mask = __ballot(pred[i] != 0);
	mbcnt[i] = wave_mbcnt(mask);
}
// get[l * n + i] = wave_get(x[i], l) (l a constant of the loop: a uniform lane index); read[l * n + i] = wave_read(x[i], lanes[l]) (the lane index is loaded from memory; it is the same in every lane, so the compiler may keep it scalar)
__global__ void __launch_bounds__(256) k_lanes(const uint32_t *x, const int *lanes, uint32_t *get, uint32_t *read, int n)
{
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	const uint32_t v = x[i];
	for (int l = 0; l < 64; l++) { get[l * n + i] = wave_get(v, l); read[l * n + i] = wave_read(v, lanes[l]); }
}
// one thread: kind 2: store_u32x2_dword_aligned(buf + at, a, b); kind 4: store_u32x4_global(buf + at, a, b, c, d)
__global__ void k_store(uint32_t *buf, int at, int kind, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
	if (threadIdx.x || blockIdx.x) return;
	if (kind == 2) store_u32x2_dword_aligned(buf + at, a, b);
	else store_u32x4_global(buf + at, a, b, c, d);
}

namespace {
struct Dev {                                             // device copies of up to four inputs and one output of n (x mult) words
	uint32_t *p[5] = { nullptr, nullptr, nullptr, nullptr, nullptr }; bool bad = false;
	uint32_t *in(int k, const uint32_t *h, size_t n) { if (!h) return nullptr; bad |= hipMalloc(&p[k], n * 4) != hipSuccess || hipMemcpy(p[k], h, n * 4, hipMemcpyHostToDevice) != hipSuccess; return p[k]; }
	uint32_t *out(size_t n) { bad |= hipMalloc(&p[4], n * 4) != hipSuccess || hipMemset(p[4], 0, n * 4) != hipSuccess; return p[4]; }
	int done(uint32_t *h, size_t n)
	{
		bad |= hipGetLastError() != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess;
		if (!bad && h) bad |= hipMemcpy(h, p[4], n * 4, hipMemcpyDeviceToHost) != hipSuccess;
		for (int k = 0; k < 5; k++) if (p[k]) (void)hipFree(p[k]);
		return bad ? -1 : 0;
	}
};
template <int OP> int run_map(const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *out, int n, int s)
{
	if (n < 1) return -1;
	Dev v; const uint32_t *da = v.in(0, a, n), *db = v.in(1, b, n), *dc = v.in(2, c, n), *dd = v.in(3, d, n); uint32_t *o = v.out(n);
	if (!v.bad) k_map<OP><<<dim3(8), dim3(256), 0, nullptr>>>(da, db, dc, dd, o, n, s);
	return v.done(out, n);
}
}

extern "C" {
#define PRIM2(NAME, OP) int prim_##NAME(const uint32_t *a, const uint32_t *b, uint32_t *out, int n) { return run_map<OP>(a, b, nullptr, nullptr, out, n, 0); }
PRIM2(pk_adds, OP_ADDS) PRIM2(pk_subs, OP_SUBS) PRIM2(pk_addw, OP_ADDW) PRIM2(pk_maxs, OP_MAXS) PRIM2(pk_mulw, OP_MULW) PRIM2(pk_lolo, OP_LOLO) PRIM2(pk_hihi, OP_HIHI)
PRIM2(rotr32, OP_ROTR) PRIM2(mul_u24, OP_MUL24)
int prim_pk_negw(const uint32_t *a, uint32_t *out, int n) { return run_map<OP_NEGW>(a, nullptr, nullptr, nullptr, out, n, 0); }
int prim_pk_sra(const uint32_t *a, int shift, uint32_t *out, int n) { return run_map<OP_SRA>(a, nullptr, nullptr, nullptr, out, n, shift); }
int prim_pk_to8(const uint32_t *v, int shift, const uint32_t *dither, uint32_t *out, int n) { return run_map<OP_TO8>(v, nullptr, dither, nullptr, out, n, shift); }
int prim_pk_to8_bytes(const uint32_t *e, const uint32_t *o, int shift1, const uint32_t *d2e, const uint32_t *d2o, uint32_t *out, int n) { return run_map<OP_TO8_BYTES>(e, o, d2e, d2o, out, n, shift1); }
int prim_byte_perm(const uint32_t *s0, const uint32_t *s1, const uint32_t *sel, uint32_t *out, int n) { return run_map<OP_PERM>(s0, s1, sel, nullptr, out, n, 0); }
// n a multiple of 4 (whole 16-byte words)
int prim_ldg32(const uint32_t *a, uint32_t *out, int n) { return run_map<OP_LDG32>(a, nullptr, nullptr, nullptr, out, n, 0); }
int prim_ldg64(const uint32_t *a, uint32_t *out, int n) { return n % 4 ? -1 : run_map<OP_LDG64>(a, nullptr, nullptr, nullptr, out, n, 0); }
int prim_ldg128(const uint32_t *a, uint32_t *out, int n) { return n % 4 ? -1 : run_map<OP_LDG128>(a, nullptr, nullptr, nullptr, out, n, 0); }

// n a multiple of 256: workgroups of four whole waves
int prim_wave_scan_mbcnt(const uint32_t *x, const uint32_t *pred, uint32_t *scan, uint32_t *mbcnt, int n)
{
	if (n < 256 || n % 256) return -1;
	Dev v; const uint32_t *dx = v.in(0, x, n), *dp = v.in(1, pred, n); uint32_t *o = v.out(2 * (size_t)n);
	if (!v.bad) k_wave<<<dim3(n / 256), dim3(256), 0, nullptr>>>(dx, dp, o, o + n);
	uint32_t *both = new uint32_t[2 * (size_t)n];
	const int rc = v.done(both, 2 * (size_t)n);
	if (!rc) for (int i = 0; i < n; i++) { scan[i] = both[i]; mbcnt[i] = both[n + i]; }
	delete[] both;
	return rc;
}
// get, read: 64 x n words (row l: every lane's view of lane l / of lane lanes[l] of its wave)
int prim_wave_get_read(const uint32_t *x, const int *lanes, uint32_t *get, uint32_t *read, int n)
{
	if (n < 256 || n % 256) return -1;
	Dev v; const uint32_t *dx = v.in(0, x, n); const int *dl = (const int *)v.in(1, (const uint32_t *)lanes, 64); uint32_t *o = v.out(128 * (size_t)n);
	if (!v.bad) k_lanes<<<dim3(n / 256), dim3(256), 0, nullptr>>>(dx, dl, o, o + 64 * (size_t)n, n);
	uint32_t *both = new uint32_t[128 * (size_t)n];
	const int rc = v.done(both, 128 * (size_t)n);
	if (!rc) for (size_t i = 0; i < 64 * (size_t)n; i++) { get[i] = both[i]; read[i] = both[64 * (size_t)n + i]; }
	delete[] both;
	return rc;
}
// buf: nwords words in and out (device memory is 256-byte aligned: word k of buf sits at byte 4 k of an aligned block); the store goes to words at .. at + kind - 1
int prim_store(uint32_t *buf, int nwords, int at, int kind, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
	if ((kind != 2 && kind != 4) || at < 0 || at + kind > nwords) return -1;
	Dev v; v.bad |= hipMalloc(&v.p[4], (size_t)nwords * 4) != hipSuccess || hipMemcpy(v.p[4], buf, (size_t)nwords * 4, hipMemcpyHostToDevice) != hipSuccess;
	if (!v.bad) k_store<<<dim3(1), dim3(64), 0, nullptr>>>(v.p[4], at, kind, a, b, c, d);
	return v.done(buf, nwords);
}
} // extern "C"
