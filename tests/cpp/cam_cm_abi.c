/* include/gsr_cam_cm.h as a C99 translation unit (tests/test_cam_cm_cpu.py compiles it with -pedantic -Werror and links it against
 * the library): the struct's fields, the two declarations, and the host-only behaviour that needs no device. */
#include <stdio.h>
#include <string.h>
#include "gsr_cam_cm.h"
#include "gsr_cam_cm.h"

int main(void)
{
	gsr_cam_cm_args c;
	gsr_camera_model m;
	gsr_backward_args a;
	int (*entry)(const gsr_backward_args*, const gsr_camera_model*, int, const float*, const gsr_aux_args*, const gsr_cam_cm_args*, int, int,
	             int) = gsr_backward_gaussians_cam_cm;
	size_t (*bytes)(int) = gsr_cam_cm_bytes;
	size_t last = 0;
	int P;
	memset(&c, 0, sizeof c);
	memset(&a, 0, sizeof a);
	m.model = GSR_CAMERA_FISHEYE; m.fx = m.fy = 10.0f; m.cx = m.cy = 8.0f;
	if (bytes(0) < 16 || bytes(-5) < 16) { printf("gsr_cam_cm_bytes is below 16 for P <= 0\n"); return 1; }
	for (P = -2; P < 4100; P++) {
		if (bytes(P) < last) { printf("gsr_cam_cm_bytes decreases at P = %d\n", P); return 1; }
		last = bytes(P);
	}
	/* cam with NULL outputs: refused under the entry point's own name, before any device work */
	a.P = 4; a.width = 16; a.height = 16;
	if (entry(&a, &m, 0, NULL, NULL, &c, 0, 4, 0) != GSR_ERR_INVALID_ARGUMENT) { printf("NULL outputs were not refused\n"); return 1; }
	if (strncmp(gsr_last_error(), "gsr_backward_gaussians_cam_cm:", 30) != 0) { printf("unexpected message: %s\n", gsr_last_error()); return 1; }
	printf("cam_cm_abi ok\n");
	return 0;
}
