/* include/gsr_knn.h as a C99 translation unit (tests/test_knn_graph_cpu.py compiles it with -pedantic -Werror and links it against
 * the library): the six declarations and the host-only behaviour that needs no device -- every refusal comes before any device work,
 * zero counts return 0 with NULL pointers, and the scratch sizes are 0 at 0 and grow. */
#include <stdio.h>
#include <string.h>
#include "gsr_knn.h"
#include "gsr_knn.h"

static int refused(int rc, const char* who, const char* what)
{
	if (rc == GSR_ERR_INVALID_ARGUMENT && strncmp(gsr_last_error(), who, strlen(who)) == 0 && gsr_last_error()[strlen(who)] == ':') return 1;
	printf("%s: %s was not refused (rc %d, text \"%s\")\n", who, what, rc, gsr_last_error());
	return 0;
}

int main(void)
{
	size_t (*sb)(int, int) = gsr_knn_search_scratch_bytes;
	int (*search)(int, const float*, int, const float*, int, float*, int*, void*, void*) = gsr_knn_search;
	size_t (*gb)(int, int) = gsr_knn_graph_scratch_bytes;
	int (*build)(int, const int*, int, int*, int*, int*, void*, void*) = gsr_knn_graph_build;
	int (*gather)(int, int, int, const float*, const int*, float*, void*) = gsr_knn_gather;
	int (*gather_bwd)(int, int, const int*, const int*, const float*, float*, void*) = gsr_knn_gather_backward;
	/* never dereferenced: every call below is refused, or has nothing to do, before any device work */
	static float f[64];
	static int i32[64];
	static char raw[64];
	char* aligned = raw + ((16 - ((size_t)raw & 15)) & 15);
	int ok = 1, n;
	size_t last;

	if (sb(0, 0) != 0 || gb(0, 0) != 0 || gb(0, 5) != 0 || gb(5, 0) != 0) { printf("scratch sizes are not 0 at 0\n"); return 1; }
	/* the areas are rounded up to 256 bytes: never smaller for a larger count, and larger over a wide step */
	for (last = 0, n = 1; n <= 70000; n = n * 3 + 1) {
		if (sb(n, 0) < last || sb(1000, n) < sb(1000, n / 3) || gb(n, 10) < gb(n / 3, 10) || sb(n, 0) == 0 || gb(n, 10) == 0) {
			printf("a scratch size shrinks or is 0 at %d\n", n); return 1;
		}
		last = sb(n, 0);
	}
	if (sb(70000, 0) <= sb(1000, 0) || sb(1000, 70000) <= sb(1000, 1000) || sb(1000, 1000) <= sb(1000, 0) || gb(70000, 10) <= gb(1000, 10)) {
		printf("a scratch size does not grow with P, Q or E\n"); return 1;
	}

	/* zero counts: 0 with NULL pointers */
	if (search(0, NULL, 0, NULL, 3, NULL, NULL, NULL, NULL) != GSR_OK) { printf("search P = 0: %s\n", gsr_last_error()); return 1; }
	if (search(5, NULL, 0, f, 3, NULL, NULL, NULL, NULL) != GSR_OK) { printf("search Q = 0: %s\n", gsr_last_error()); return 1; }
	if (search(0, NULL, 7, f, 3, NULL, NULL, NULL, NULL) != GSR_OK) { printf("search P = 0, Q = 7: %s\n", gsr_last_error()); return 1; }
	if (build(0, NULL, 0, NULL, NULL, NULL, NULL, NULL) != GSR_OK) { printf("graph_build E = 0: %s\n", gsr_last_error()); return 1; }
	if (gather(0, 4, 3, NULL, NULL, NULL, NULL) != GSR_OK || gather(4, 0, 3, NULL, NULL, NULL, NULL) != GSR_OK ||
	    gather(4, 4, 0, NULL, NULL, NULL, NULL) != GSR_OK) { printf("gather with a zero count: %s\n", gsr_last_error()); return 1; }
	if (gather_bwd(0, 3, NULL, NULL, NULL, NULL, NULL) != GSR_OK || gather_bwd(3, 0, NULL, NULL, NULL, NULL, NULL) != GSR_OK) {
		printf("gather_backward with a zero count: %s\n", gsr_last_error()); return 1;
	}

	/* refusals */
	ok &= refused(search(-1, f, -1, NULL, 3, f, i32, aligned, NULL), "gsr_knn_search", "a negative P");
	ok &= refused(search(4, f, -2, f, 3, f, i32, aligned, NULL), "gsr_knn_search", "a negative Q");
	ok &= refused(search(4, f, 4, NULL, 0, f, i32, aligned, NULL), "gsr_knn_search", "K = 0");
	ok &= refused(search(4, f, 4, NULL, 33, f, i32, aligned, NULL), "gsr_knn_search", "K = 33");
	ok &= refused(search(4, f, 4, NULL, -3, f, i32, aligned, NULL), "gsr_knn_search", "K = -3");
	ok &= refused(search(4, f, 3, NULL, 3, f, i32, aligned, NULL), "gsr_knn_search", "Q != P in the self-set form");
	ok &= refused(search(4, NULL, 4, NULL, 3, f, i32, aligned, NULL), "gsr_knn_search", "points NULL");
	ok &= refused(search(4, f, 4, NULL, 3, NULL, i32, aligned, NULL), "gsr_knn_search", "dist2 NULL");
	ok &= refused(search(4, f, 4, NULL, 3, f, NULL, aligned, NULL), "gsr_knn_search", "idx NULL");
	ok &= refused(search(4, f, 4, NULL, 3, f, i32, NULL, NULL), "gsr_knn_search", "scratch NULL");
	ok &= refused(search(4, f, 4, NULL, 3, f, i32, aligned + 4, NULL), "gsr_knn_search", "unaligned scratch");
	ok &= refused(build(-1, i32, 4, i32, i32, NULL, aligned, NULL), "gsr_knn_graph_build", "a negative E");
	ok &= refused(build(4, i32, -1, i32, i32, NULL, aligned, NULL), "gsr_knn_graph_build", "a negative P");
	ok &= refused(build(4, NULL, 4, i32, i32, NULL, aligned, NULL), "gsr_knn_graph_build", "idx NULL");
	ok &= refused(build(4, i32, 4, NULL, i32, NULL, aligned, NULL), "gsr_knn_graph_build", "offsets NULL");
	ok &= refused(build(4, i32, 4, i32, NULL, NULL, aligned, NULL), "gsr_knn_graph_build", "edges NULL");
	ok &= refused(build(4, i32, 4, i32, i32, NULL, NULL, NULL), "gsr_knn_graph_build", "scratch NULL");
	ok &= refused(build(4, i32, 4, i32, i32, NULL, aligned + 8, NULL), "gsr_knn_graph_build", "unaligned scratch");
	ok &= refused(gather(-1, 2, 3, f, i32, f, NULL), "gsr_knn_gather", "a negative Q");
	ok &= refused(gather(2, -1, 3, f, i32, f, NULL), "gsr_knn_gather", "a negative K");
	ok &= refused(gather(2, 2, -3, f, i32, f, NULL), "gsr_knn_gather", "a negative C");
	ok &= refused(gather(2, 2, 3, NULL, i32, f, NULL), "gsr_knn_gather", "x NULL");
	ok &= refused(gather(2, 2, 3, f, NULL, f, NULL), "gsr_knn_gather", "idx NULL");
	ok &= refused(gather(2, 2, 3, f, i32, NULL, NULL), "gsr_knn_gather", "out NULL");
	ok &= refused(gather_bwd(-1, 3, i32, i32, f, f, NULL), "gsr_knn_gather_backward", "a negative P");
	ok &= refused(gather_bwd(2, -3, i32, i32, f, f, NULL), "gsr_knn_gather_backward", "a negative C");
	ok &= refused(gather_bwd(2, 3, NULL, i32, f, f, NULL), "gsr_knn_gather_backward", "offsets NULL");
	ok &= refused(gather_bwd(2, 3, i32, NULL, f, f, NULL), "gsr_knn_gather_backward", "edges NULL");
	ok &= refused(gather_bwd(2, 3, i32, i32, NULL, f, NULL), "gsr_knn_gather_backward", "grad_out NULL");
	ok &= refused(gather_bwd(2, 3, i32, i32, f, NULL, NULL), "gsr_knn_gather_backward", "grad_x NULL");
	if (!ok) return 1;
	printf("knn_abi_check ok: K up to %d\n", GSR_KNN_MAX_K);
	return 0;
}
