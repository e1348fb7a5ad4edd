// The scoring of an emulator run (narrow_emul, wave_emul, pipe_emul): the three presets in turn, or ONE scoring for every pair, given on
// the command line as the trailing words `scoring a b q e q2 e2 sc_ambi` -- the caller's order of the two gap models, unswapped, b as a
// penalty.  The kernel's constants come from gd_derive_consts (ksw_common.h), the function the driver calls; the oracle gets the caller's
// order and sc_ambi in its matrix, and reports emu.score + score_bias (see ksw_score_bias_kernel).
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ksw_common.h"

static const int EMU_PRESETS[3][7] = {{2, 8, 12, 2, 24, 1, 0}, {1, 4, 6, 2, 26, 1, 0}, {2, 4, 4, 2, 24, 1, 0}}; // sr, hifi, ont

// true: P holds the scoring of the command line; argc is cut back to the words before it
static inline bool emu_scoring_arg(int &argc, char **argv, int P[7])
{
	for (int i = 1; i < argc; ++i)
		if (!strcmp(argv[i], "scoring")) {
			if (i + 8 != argc) { fprintf(stderr, "usage: ... scoring a b q e q2 e2 sc_ambi\n"); exit(2); }
			for (int k = 0; k < 7; ++k) P[k] = atoi(argv[i + 1 + k]);
			argc = i;
			return true;
		}
	return false;
}

// single: the single-affine form, ksw_extz2(q, e) -- the kernel's constants are those of (q, e, q, e), as gdiet_hip_ksw_extz2_batch passes them
static inline KswDerived emu_consts(const int P[7], bool single, int8_t mat[25])
{
	for (int i = 0; i < 25; ++i) mat[i] = (i / 5 == 4 || i % 5 == 4) ? P[6] : (i / 5 == i % 5 ? P[0] : -P[1]);
	return gd_derive_consts(P[0], -P[1], P[6], P[2], P[3], single ? P[2] : P[4], single ? P[3] : P[5]);
}
