/*
 * ref_bm_cl.c -- runs the reference's own block-matching OpenCL text (OptFlow_C1_D0, Histogram_C1_D0) on the CPU.
 * TEST INFRASTRUCTURE ONLY; built into oracle/_ref/ (never committed) and only where the reference checkout exists.
 *
 * The text is included from the checkout through REF_BM_CL (a -D path, see oracle/Makefile); nothing of it is copied here.
 * It is plain enough C that an address-space shim and cl_host.h's built-ins are all it needs.
 *
 * Launch geometry as the reference's host sets it up (FastSpacedBMMethod_OCL.cpp:90-145):
 *   OptFlow    groups = grid = ((w - 2r) / (block + step), (h - 2r) / (block + step)), local = scan_block x scan_block
 *   Histogram  one group, local = grid
 *   both image offsets 0, imgSrcWidth = w (a dense frame), imgDstWidth = grid_x, TestDepth = 3
 * OptFlow's work-groups run one after another (one instance of its __local arrays at a time, barrier() per group).
 */
#include <math.h>
#include <stdbool.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define CLH_PLAIN_NAMES
#include "cl_host.h"

#define __kernel
#define __global
#define __constant const
#define __local static

#ifndef REF_BM_CL
#error "REF_BM_CL must name the reference's FastSpacedBMMethod.cl"
#endif
#include REF_BM_CL

#define REF_ARRAY 50 /* the text's arraySize: its __local arrays hold diameters up to 49 */

typedef struct {
  const unsigned char *cur, *prev;
  int w, grid_x, block, step, radius;
  signed char *dx, *dy;
  signed char value_x, value_y, out9x[9], out9y[9];
} bm_args;

static void run_optflow(void* p) {
  bm_args* a = (bm_args*)p;
  OptFlow_C1_D0(a->cur, a->prev, a->w, 0, a->grid_x, 0, a->dx, a->dy, a->block, a->step, a->radius);
}

static void run_histogram(void* p) {
  bm_args* a = (bm_args*)p;
  Histogram_C1_D0(a->dx, a->dy, a->grid_x, 0, a->radius, 2 * a->radius + 1, &a->value_x, &a->value_y, 3, a->out9x, a->out9y);
}

/* dx, dy: [grid_y * grid_x] per-block shifts; out9x, out9y: the kernel's nine (x, y) candidates, x = out9x[3 i + j] = i-th
 * most frequent x, y = out9y[3 i + j] = j-th most frequent y. Returns 0, -1 on a geometry the text's arrays cannot hold. */
int ref_bm_cl(const uint8_t* cur, const uint8_t* prev, int w, int h, int block, int step, int radius, int scan_block,
              int8_t* dx, int8_t* dy, int8_t* out9x, int8_t* out9y) {
  if (!cur || !prev || !dx || !dy || !out9x || !out9y) return -1;
  if (block < 1 || step < 0 || radius < 1 || 2 * radius + 1 >= REF_ARRAY || scan_block < 1 || scan_block > 2 * radius + 1) return -1;
  const int gx = (w - 2 * radius) / (block + step), gy = (h - 2 * radius) / (block + step);
  if (gx < 1 || gy < 1) return -1;
  bm_args a;
  memset(&a, 0, sizeof(a));
  a.cur = cur; a.prev = prev; a.w = w; a.grid_x = gx; a.block = block; a.step = step; a.radius = radius;
  a.dx = (signed char*)dx; a.dy = (signed char*)dy;
  const size_t grid[2] = {(size_t)gx, (size_t)gy}, local[2] = {(size_t)scan_block, (size_t)scan_block};
  const size_t one[2] = {1, 1}, zero[2] = {0, 0};
  for (size_t by = 0; by < grid[1]; ++by)
    for (size_t bx = 0; bx < grid[0]; ++bx) {
      const size_t first[2] = {bx, by};
      if (clh_launch(run_optflow, &a, grid, local, first, one, 0)) return -2;
    }
  if (clh_launch(run_histogram, &a, one, grid, zero, one, 0)) return -2;
  memcpy(out9x, a.out9x, 9);
  memcpy(out9y, a.out9y, 9);
  return 0;
}
