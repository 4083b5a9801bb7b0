// aa_rho.cpp -- the opacity compensation of the anti-aliased path (csrc/gsr_aa.h: gsr_aa_rho, gsr_aa_rho_grad), run on the host: for
// every "a b c" triple of hex floats on stdin prints "rho drho_da drho_db drho_dc rho2" as hex floats (rho2: gsr_aa_rho, which must equal
// rho).  tests/test_antialias_cpu.py compiles it -ffp-contract=off like the two kernels and compares it with float64 autograd.
#include <cstdio>
#include "../../gaussian-splatting_cc-comments_amd/csrc/gsr_aa.h"

int main()
{
	float a, b, c;
	while (scanf("%a %a %a", &a, &b, &c) == 3) {
		const GsrAAGrad g = gsr_aa_rho_grad(a, b, c);
		printf("%a %a %a %a %a\n", g.rho, g.drho_da, g.drho_db, g.drho_dc, gsr_aa_rho(a, b, c));
	}
	return 0;
}
