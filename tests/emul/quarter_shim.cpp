// The first rung of the 64-lane DP kernel's ladder behind a C entry, for tests/quarter_pairs.py: the band at which a box runs the
// quarter-block rows first (gd_quarter_rung, the function the kernel evaluates, on the planner's own mark), and the constant.
//   g++ -O2 -std=c++17 -shared -fPIC -I genome-on-diet_amd/csrc tests/emul/quarter_shim.cpp -o libquarter_shim.so
#define __host__
#define __device__
#include "ksw_plan.h"

extern "C" int quarter_w(void) { return GD_W_QUARTER; }
// 0: no quarter rung for this box; otherwise its band (== w: the box's own band, nothing to certify)
extern "C" int quarter_planned_rung(int qlen, int tlen, int w)
{
	int32_t kind, row_bytes;
	gd_plan_one(GdPlanOpt(), qlen, tlen, w, kind, row_bytes);
	if (kind != GD_KIND_WAVE64) return 0;
	const int wa = w < 0 ? (tlen > qlen ? tlen : qlen) : w;
	return gd_quarter_rung(gd_narrow_mode(qlen, tlen, w), qlen, tlen, wa, GD_W_QUARTER);
}
extern "C" int quarter_break_even_num(void) { return GD_QUARTER_BREAK_EVEN_NUM; }
extern "C" int quarter_break_even_den(void) { return GD_QUARTER_BREAK_EVEN_DEN; }
