/* mamg_test.h -- test and verification hooks of libmamg.so.
 *
 * Not part of the preconditioner API (include/mamg.h): no reference
 * counterpart, no stability promise.  The tests and the A/B scripts use them;
 * a caller of the metric_mono path never needs them. */
#ifndef MAMG_TEST_H
#define MAMG_TEST_H
#include "mamg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Set (value != NULL)
 * or reset (NULL) one of the library's internal layout switches for the
 * process (names in mamg_option_names(); DESIGN.md section 4 gives the
 * measured defaults).  The product library reads no environment variables;
 * MAMG_ERR_ARG for an unknown name.
 * Every setup call reads the switches once, at its entry: a call here
 * affects the handles set up after it, and a handle keeps the switches it was
 * built with for life (its layouts, its first apply and every later one). */
int mamg_set_option(const char* name, const char* value);
const char* mamg_option_names(void);   /* comma-separated */

/* The switches a handle was built with, as "NAME=value" joined by commas in
 * mamg_option_names() order.  Values are the resolved ones (defaults spelled
 * out, clamps applied; "auto" / empty where an unset switch is a state of its
 * own).  h == NULL: what a setup starting now would read (needs no GPU).
 * MAMG_ERR_ARG when cap cannot hold the text and its terminator. */
int mamg_handle_options(const mamg_handle* h, char* buf, int64_t cap);
int mamg_dist_options(const mamg_dhandle* h, char* buf, int64_t cap);

/* Verification of a row-sharded Galerkin product (the start of a
 * partition-local setup): on nranks
 * virtual ranks (fine nodes and coarse nodes split into even ranges), rank p
 * forms its (A P) rows from its A rows and the P rows of the fine dofs they
 * reach (its own and a halo), then its coarse rows of R (A P), R = P^T, from
 * its R rows and the (A P) rows of the fine dofs those reach, each taken from
 * the owner rank's sharded result; the GPU setup's own SpGEMM throughout.
 * A, P, Ac: one level's field-major 2-function operator, prolongator and the
 * hierarchy's next-level operator (host CSR).  res6: (A P) rows differing
 * from the unsharded product, A_c rows differing from Ac (bitwise), halo P
 * rows read, halo (A P) rows read, (A P) rows and A_c rows compared. */
int mamg_sharded_galerkin_check(const mamg_csr* A, const mamg_csr* P, const mamg_csr* Ac, int nranks, int device,
                                int64_t* res6);

/* Which plan the coarse tail's planner took for a handle (DESIGN.md section
 * 4.2): the index-th cached tail program (one per (b, x) entry of tail_level:
 * a V-cycle has one, a W-cycle's second visit a second one).  Programs are
 * planned at the first apply.  Writes up to cap values and returns how many
 * the program has (call again with a larger cap if it exceeds cap), 0 when no
 * program index exists (nothing planned yet, the tail is off, or it was
 * refused: info[0], info[1] and info[11] are still written), MAMG_ERR_ARG for
 * a bad argument.  info[]:
 *   0 cached programs        1 tail_level (0: no tail)
 *   2 ops of the program     3 dynamic LDS bytes of its launch
 *   4 xl: every gathered x in LDS (1 / 0)
 *   5 res: register-resident rows (1 / 0)
 *   6 prog_lds: LDS byte offset of the op descriptors, -1: read from global
 *   7 resident rows          8 overflow blocks of rows longer than 12 (nov)
 *   9 vector operands tagged LDS     10 vector operands in global memory
 *     (of every op but the copies in and out and the row load)
 *  11 the planner refused the last attempt (an op the tail cannot express;
 *     the level then runs as launches)
 *  12 dense solves (T_GEMV ops)
 *  13 SpMV / GS ops run from resident rows   14 ... run from global arrays
 *  15 largest lane count of the ops in 14
 *  16 a residency plan was made and discarded (its LDS region did not fit next
 *     to the vectors; values 5, 7, 8 then describe the replanned program)
 *  17 nonlinear AMLI step ops (T_KDOT / T_KORTH / T_KUPD; mamg_set_kcycle_tail);
 *     their operands count in 9 and 10
 *  18.. per dense solve: n, 1 if its matrix is in the LDS region (else global) */
int mamg_tail_info(const mamg_handle* h, int index, int64_t* info, int cap);

/* Thresholds of the row-pattern dictionary of a level-0 A (DESIGN.md section
 * 3), for the process: the node rows from which it is tried, the cap on row
 * types, and the bits kept of a row's hash (a few bits force collisions; the
 * layout must then be refused or exact).  A negative value restores that
 * default.  Read by every setup at its entry, with the switches. */
int mamg_test_set_rowdict(int64_t min_rows, int max_types, int hash_bits);

/* What the dictionary's builder decided for the handle's level-0 A.  Writes
 * up to cap values, returns how many there are (5), MAMG_ERR_ARG for a bad
 * argument.  info[]:
 *   0 taken (1 / 0)
 *   1 refusal reason: 0 none, 1 more row types than the cap, 2 a row longer
 *     than 32 blocks, 3 the verification pass found a difference, 4 fewer
 *     rows than the threshold, 5 not square, 6 the table exceeds 64 KB,
 *     7 not tried (the handle holds the CSR layout)
 *   2 row types found (past the cap: as many as were counted before the stop)
 *   3 longest row in blocks      4 bytes of the type table */
int mamg_rowdict_info(const mamg_handle* h, int64_t* info, int cap);

/* The matrix-free level-0 post step, for the process:
 * mode 0 never takes it, any other mode takes it where eligible (negative:
 * the default, which is on); min_rows is the node rows of level 0 from which
 * it is taken (negative: the default, 1 << 22).  A threshold of its own, not
 * the dictionary's: lowering only the dictionary's keeps the stored K.  Read
 * by every setup at its entry, with the switches. */
int mamg_test_set_post_mf(int mode, int64_t min_rows);

/* What the layout builder decided for the handle's level-0 post step.  Writes
 * up to cap values, returns how many there are (3), MAMG_ERR_ARG for a bad
 * argument.  info[]:
 *   0 taken (1 / 0)
 *   1 refusal reason: 0 none, 1 switched off (mode 0), 2 fewer rows than the
 *     threshold, 3 level-0 A is not a row dictionary, 4 the prolongator is not
 *     (I - w D_B^-1 A) T (AMG_type is not SA with sa_block_diag, or the setup
 *     handed no aggregates over), 5 the smoother is not Jacobi-like (GS / SGS,
 *     patches, rings), 6 post_fusion is off or there is no post sweep, 7 not
 *     tried (CSR layout or a single level), 8 a row type without a positive
 *     diagonal block
 *   2 bytes of the per-type table Wp = w D_B^-1 */
int mamg_post_mf_info(const mamg_handle* h, int64_t* info, int cap);

/* Where the GPU setups run the Vanek-Mandel-Brezina aggregation
 * (aggregation_type VMB), for the process.
 *   mode 1, the default: on the device, by worklist rounds that reach the
 *     sequential loop's aggregates exactly, on levels of at least 131072
 *     nodes; smaller levels, where the rounds measured slower than the round
 *     trip, send the strong graph to the host and run the loop there;
 *   mode 2: on the device whatever the level's size (tests);
 *   mode 0: on the host.
 * Every path gives the same hierarchy bit for bit.  max_rounds: the device
 * rounds of one level after which that level is abandoned to the host path;
 * a negative value restores the default rule (the rounds that cost what the
 * host path would, from the graph's entries).  Read by every setup at its
 * entry, with the switches.  MAMG_ERR_ARG for another mode. */
int mamg_test_set_vmb(int mode, int64_t max_rounds);

/* What the VMB aggregation of one level did in the calling thread's most
 * recent GPU setup.  Writes up to cap values, returns how many there are (8),
 * 0 when that level ran no VMB aggregation, MAMG_ERR_ARG for a bad argument.
 * info[]:
 *   0 path: 0 host by request, 1 device, 2 device abandoned at the round cap,
 *     then host, 3 host because the level is below the size threshold
 *   1 device rounds (path 2: those run before the cap)
 *   2 root-rule evaluations summed over the rounds
 *   3 roots (aggregates)         4 non-isolated nodes
 *   5 nodes joined in phase 2 (to their strongest aggregated neighbour)
 *     (3 and 5: path 1 only; 4: paths 1 and 2; 0 otherwise)
 *   6 bytes the aggregation step copied to the host (after the strength
 *     graph is built: the round counters, or the graph itself)
 *   7 microseconds of that step, to the aggregate numbers in device memory
 *     (bench/vmb_setup.py: cost per round and the host path's time per level) */
int mamg_test_vmb_info(int level, int64_t* info, int cap);

#ifdef __cplusplus
}
#endif
#endif /* MAMG_TEST_H */
