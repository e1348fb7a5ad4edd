// The narrow-band certificate of the 64-lane DP kernel (gd_band_certified, ksw_wave_core.h) behind a C entry, for tests/test_band_certificate.py:
// the very function the kernel evaluates, with the constants the driver derives (gd_narrow_arg).
//   g++ -O2 -std=c++17 -shared -fPIC -I genome-on-diet_amd/csrc tests/emul/cert_shim.cpp -o libcert_shim.so
#define __host__
#define __device__
#include "ksw_plan.h"

extern "C" int cert_w_narrow(void) { return GD_W_NARROW; }
// scoring as gd_consts normalises it (q + e <= q2 + e2; sc_mis, sc_N as scores); 1: the alignment at band w is the alignment at any wider band
extern "C" int cert_band_certified(int w, int sc_mch, int sc_mis, int sc_N, int q, int e, int q2, int e2, int qlen, int tlen, int score)
{
	KswConst C;
	C.q = q, C.e = e, C.q2 = q2, C.e2 = e2, C.sc_mch = sc_mch, C.sc_mis = sc_mis, C.sc_N = sc_N, C.long_thres = 0, C.long_diff = 0;
	return gd_band_certified(gd_narrow_arg(C, w), qlen, tlen, score) ? 1 : 0;
}
// ... and from a scoring as the CALLER passes it (mismatch, sc_ambi as scores; the gap models in the caller's order), through the driver's own
// derivation (gd_derive_consts, ksw_common.h).  `score` is the kernel's, unshifted: what the library reports minus cert_score_bias.
extern "C" int cert_certified_for(int w, int match, int mismatch, int sc_ambi, int q, int e, int q2, int e2, int qlen, int tlen, int score)
{
	return gd_band_certified(gd_narrow_arg(gd_derive_consts(match, mismatch, sc_ambi, q, e, q2, e2).K, w), qlen, tlen, score) ? 1 : 0;
}
extern "C" int cert_score_bias(int match, int mismatch, int sc_ambi, int q, int e, int q2, int e2)
{
	return gd_derive_consts(match, mismatch, sc_ambi, q, e, q2, e2).score_bias;
}
extern "C" int cert_narrow_mode(int qlen, int tlen, int w) { return gd_narrow_mode(qlen, tlen, w); }
// ... and the mark of a box as the planner sets it (default options): only the 64-lane kernel's boxes carry one
extern "C" int cert_planned_mode(int qlen, int tlen, int w)
{
	int32_t kind, row_bytes;
	gd_plan_one(GdPlanOpt(), qlen, tlen, w, kind, row_bytes);
	return kind == GD_KIND_WAVE64 ? gd_narrow_mode(qlen, tlen, w) : GD_NARROW_NO;
}
