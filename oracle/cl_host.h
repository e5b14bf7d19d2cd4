/*
 * cl_host.h -- a CPU host for OpenCL C program text: a cooperative work-item scheduler and the handful of OpenCL built-ins
 * that the reference's block-matching kernels and the peak stage of its FFT kernel use. TEST INFRASTRUCTURE ONLY.
 *
 * It exists so that the oracle's restatements can be held to the reference's own program text, executed, instead of to a
 * reading of it. The text itself is never copied: oracle/ref_bm_cl.c includes it through a -D path, oracle/ref_fft_peak.cpp
 * links an object that clang compiled from it in OpenCL mode (see the `ref` target of oracle/Makefile).
 *
 * Execution model
 *   clh_launch() runs a set of work-groups. Every work-item is a ucontext coroutine on a stack of its own; the scheduler
 *   resumes the live work-items in ascending order (group row-major, then local id row-major), and a work-item runs until
 *   it calls barrier() or returns. One pass over the live work-items is therefore one barrier phase. The run is single
 *   threaded and deterministic: between two barriers the work-items execute one after another in that order, which is one
 *   of the interleavings OpenCL allows for race-free text.
 *
 *   barrier() synchronises EVERY work-item handed to one clh_launch() call, not the work-items of one group. This is the
 *   reading the oracle documents for the reference's FFT kernel (pc_ref_impl.h, "the race-free reading"): that kernel
 *   exchanges data between work-groups across barrier(), which OpenCL does not guarantee, so its intended result is the one
 *   a launch-wide barrier gives. A driver that wants OpenCL's own per-group barrier -- and one instance of the text's
 *   __local (here: static) arrays at a time -- passes one group per call (group_first/group_count below), as ref_bm_cl.c
 *   does: work-groups then run one after another.
 *
 *   A work-item that returns early simply leaves the rotation; the others' barriers do not wait for it (the behaviour of
 *   every real implementation, and what OptFlow_C1_D0's early return relies on).
 *
 * Two ways to bind the built-ins
 *   CLH_PLAIN_NAMES     the text is #included into a C translation unit behind the driver's own address-space shim: the
 *                       built-ins are ordinary C functions / macros (get_group_id, barrier, atomic_add, ...).
 *   CLH_MANGLED_NAMES   the text was compiled by clang -x cl into an object: its built-ins are overloadable, so the object
 *                       refers to them by their Itanium-mangled names; they are defined here through asm labels (which
 *                       also covers the ones whose mangling carries an address space, vload2 / vstore2).
 * Both produce float results with the plain C operators; build with -ffp-contract=off so that mad()/fma() below are the
 * only fused operations (fma is correctly rounded by definition; mad is evaluated as a*b+c unfused, one of the results
 * OpenCL permits and the one the oracle's float model assumes on a target without FMA).
 */
#ifndef MOF_ORACLE_CL_HOST_H
#define MOF_ORACLE_CL_HOST_H

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <ucontext.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void (*clh_kernel_fn)(void* arg);

typedef struct clh_item {
  ucontext_t ctx;
  size_t group[2], local[2];
  int done;
} clh_item;

static struct {
  ucontext_t sched;
  clh_item* items;
  clh_item* cur;
  size_t local_size[2], num_groups[2];
  clh_kernel_fn fn;
  void* arg;
} clh_state;

static inline size_t clh_get_group_id(unsigned d) { return d < 2 ? clh_state.cur->group[d] : 0; }
static inline size_t clh_get_local_id(unsigned d) { return d < 2 ? clh_state.cur->local[d] : 0; }
static inline size_t clh_get_local_size(unsigned d) { return d < 2 ? clh_state.local_size[d] : 1; }
static inline size_t clh_get_num_groups(unsigned d) { return d < 2 ? clh_state.num_groups[d] : 1; }
static inline size_t clh_get_global_id(unsigned d) { return clh_get_group_id(d) * clh_get_local_size(d) + clh_get_local_id(d); }
static inline size_t clh_get_global_size(unsigned d) { return clh_get_num_groups(d) * clh_get_local_size(d); }

/* launch-wide barrier: hand control back to the scheduler, which resumes this work-item in the next phase */
static inline void clh_barrier(void) { swapcontext(&clh_state.cur->ctx, &clh_state.sched); }

static void clh_trampoline(void) {
  clh_state.fn(clh_state.arg);
  clh_state.cur->done = 1; /* uc_link returns to the scheduler */
}

/* (getcontext may return twice as far as the compiler knows: kept out of the loops of clh_launch) */
static __attribute__((noinline)) void clh_item_start(clh_item* it, char* stack, size_t stack_bytes) {
  getcontext(&it->ctx);
  it->ctx.uc_stack.ss_sp = stack;
  it->ctx.uc_stack.ss_size = stack_bytes;
  it->ctx.uc_link = &clh_state.sched;
  makecontext(&it->ctx, clh_trampoline, 0);
}

/* Runs fn(arg) once per work-item of the groups [group_first, group_first + group_count) of an NDRange of num_groups groups of
 * local_size work-items (two dimensions; dimension 0 is the fastest). Returns 0, or -1 on a bad geometry / allocation failure.
 * stack_bytes is each work-item's stack (0: 64 KiB, ample for text that keeps its arrays in __local / __global memory). */
static int clh_launch(clh_kernel_fn fn, void* arg, const size_t num_groups[2], const size_t local_size[2],
                      const size_t group_first[2], const size_t group_count[2], size_t stack_bytes) {
  if (!fn || !num_groups[0] || !num_groups[1] || !local_size[0] || !local_size[1] || !group_count[0] || !group_count[1]) return -1;
  if (group_first[0] + group_count[0] > num_groups[0] || group_first[1] + group_count[1] > num_groups[1]) return -1;
  if (!stack_bytes) stack_bytes = 64 * 1024;
  const size_t per_group = local_size[0] * local_size[1];
  const size_t count = group_count[0] * group_count[1] * per_group;
  clh_item* items = (clh_item*)calloc(count, sizeof(clh_item));
  char* stacks = (char*)malloc(count * stack_bytes);
  if (!items || !stacks) { free(items); free(stacks); return -1; }
  clh_state.items = items;
  clh_state.fn = fn;
  clh_state.arg = arg;
  for (int d = 0; d < 2; ++d) { clh_state.local_size[d] = local_size[d]; clh_state.num_groups[d] = num_groups[d]; }
  size_t k = 0;
  for (size_t gy = 0; gy < group_count[1]; ++gy)
    for (size_t gx = 0; gx < group_count[0]; ++gx)
      for (size_t ly = 0; ly < local_size[1]; ++ly)
        for (size_t lx = 0; lx < local_size[0]; ++lx, ++k) {
          clh_item* it = &items[k];
          it->group[0] = group_first[0] + gx; it->group[1] = group_first[1] + gy;
          it->local[0] = lx; it->local[1] = ly;
          clh_item_start(it, stacks + k * stack_bytes, stack_bytes);
        }
  for (size_t live = count; live;) {
    live = 0;
    for (k = 0; k < count; ++k) {
      if (items[k].done) continue;
      clh_state.cur = &items[k];
      swapcontext(&clh_state.sched, &items[k].ctx);
      if (!items[k].done) ++live;
    }
  }
  clh_state.cur = NULL;
  clh_state.items = NULL;
  free(stacks);
  free(items);
  return 0;
}

#ifdef __cplusplus
}
#endif

/* ---- built-ins under their plain names (text #included into C) ------------------------------------------------------ */
#ifdef CLH_PLAIN_NAMES
#define CLK_LOCAL_MEM_FENCE 1
#define CLK_GLOBAL_MEM_FENCE 2
#define get_group_id(d) ((int)clh_get_group_id(d))
#define get_local_id(d) ((int)clh_get_local_id(d))
#define get_local_size(d) ((int)clh_get_local_size(d))
#define get_num_groups(d) ((int)clh_get_num_groups(d))
#define barrier(flags) clh_barrier()
/* int atomics on __local / __global memory; both return the old value */
#define atomic_add(p, v) __atomic_fetch_add((p), (v), __ATOMIC_SEQ_CST)
#define atomic_xchg(p, v) __atomic_exchange_n((p), (v), __ATOMIC_SEQ_CST)
#endif

/* ---- built-ins under the names a clang -x cl object refers to (x86-64, Itanium mangling) ----------------------------- */
#ifdef CLH_MANGLED_NAMES
#define CLH_SYM(name) __asm__(name)
#ifdef __cplusplus
extern "C" {
#endif
typedef float clh_float2 __attribute__((vector_size(8))); /* OpenCL's float2 as x86-64 passes it: one SSE register */

size_t clh_m_get_group_id(unsigned d) CLH_SYM("_Z12get_group_idj");
size_t clh_m_get_local_id(unsigned d) CLH_SYM("_Z12get_local_idj");
size_t clh_m_get_local_size(unsigned d) CLH_SYM("_Z14get_local_sizej");
size_t clh_m_get_num_groups(unsigned d) CLH_SYM("_Z14get_num_groupsj");
size_t clh_m_get_global_id(unsigned d) CLH_SYM("_Z13get_global_idj");
size_t clh_m_get_global_size(unsigned d) CLH_SYM("_Z15get_global_sizej");
void clh_m_barrier(unsigned flags) CLH_SYM("_Z7barrierj");
int clh_m_mad24(int a, int b, int c) CLH_SYM("_Z5mad24iii");
int clh_m_mul24(int a, int b) CLH_SYM("_Z5mul24ii");
unsigned clh_m_min_uu(unsigned a, unsigned b) CLH_SYM("_Z3minjj");
float clh_m_ceil(float a) CLH_SYM("_Z4ceilf");
float clh_m_fma(float a, float b, float c) CLH_SYM("_Z3fmafff");
float clh_m_mad(float a, float b, float c) CLH_SYM("_Z3madfff");
float clh_m_rsqrt(float a) CLH_SYM("_Z5rsqrtf");
clh_float2 clh_m_vload2(size_t offset, const float* p) CLH_SYM("_Z6vload2mPU8CLglobalKf");
void clh_m_vstore2(clh_float2 v, size_t offset, float* p) CLH_SYM("_Z7vstore2Dv2_fmPU8CLglobalf");

size_t clh_m_get_group_id(unsigned d) { return clh_get_group_id(d); }
size_t clh_m_get_local_id(unsigned d) { return clh_get_local_id(d); }
size_t clh_m_get_local_size(unsigned d) { return clh_get_local_size(d); }
size_t clh_m_get_num_groups(unsigned d) { return clh_get_num_groups(d); }
size_t clh_m_get_global_id(unsigned d) { return clh_get_global_id(d); }
size_t clh_m_get_global_size(unsigned d) { return clh_get_global_size(d); }
void clh_m_barrier(unsigned flags) { (void)flags; clh_barrier(); }
/* the text's operands are far inside 24 bits, where mad24 / mul24 are the plain integer expressions */
int clh_m_mad24(int a, int b, int c) { return a * b + c; }
int clh_m_mul24(int a, int b) { return a * b; }
unsigned clh_m_min_uu(unsigned a, unsigned b) { return b < a ? b : a; }
float clh_m_ceil(float a) { return __builtin_ceilf(a); }
float clh_m_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
float clh_m_mad(float a, float b, float c) { return a * b + c; }
float clh_m_rsqrt(float a) { return 1.0f / __builtin_sqrtf(a); }
clh_float2 clh_m_vload2(size_t offset, const float* p) { clh_float2 v = {p[2 * offset], p[2 * offset + 1]}; return v; }
void clh_m_vstore2(clh_float2 v, size_t offset, float* p) { p[2 * offset] = v[0]; p[2 * offset + 1] = v[1]; }
#ifdef __cplusplus
}
#endif
#endif /* CLH_MANGLED_NAMES */

#endif
