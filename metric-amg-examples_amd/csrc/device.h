// device.h -- device hierarchy interface (no HIP types; implemented in device.hip and, the
// multi-GPU part, in dist_layout.hip and dist_apply.hip)
#pragma once
#include <mutex>
#include <string>

#include "gsetup.h"
#include "host.h"

namespace mamg {

struct DeviceHandle;

// sw: the setup's snapshot of the switch table (opts.h); the handle keeps it
int dev_upload(const Hierarchy& H, const CsrView& A0, const mamg_params& p, const Switches& sw,
               DeviceHandle** out, std::string* err);
// apply handle from a GPU-setup hierarchy (everything stays in HBM); G's
// buffers are released level by level as the apply layouts are built
void dev_prereserve(int device, int64_t nnz, int nranks, const Switches& sw);
void dev_prereserve_release();
int dev_from_ghier(GHier* G, const DevMat& A0, const mamg_params& p, DeviceHandle** out,
                   std::string* err);
// setup phase timings of a handle built by the GPU setup (ms; zeros otherwise)
void dev_setup_ms(const DeviceHandle* h, double* ms8);
// apply-layout phases (ms): build, K value region trials, operator re-homing, finish
void dev_layout_ms(const DeviceHandle* h, double* ms4);
void dev_destroy(DeviceHandle* h);
// release the cached blocks of the setup temporaries (dmem.h tmp_trim_all)
void dev_tmp_trim();
// held across the library's stream captures and its setups (device.hip)
std::recursive_mutex& capture_mutex();
// the end of a setup: idle cached blocks above the cache limit freed
void dev_tmp_trim_to_limit();
// cache limit (bytes per device; < 0 default = HBM / 8, 0 = release every setup)
void dev_set_cache_limit(int64_t bytes);
int64_t dev_cache_limit(int device);
// idle cached bytes of a device (idle temporaries + the SpGEMM staging block)
int64_t dev_cache_idle_bytes(int device);
int64_t dev_nrows(const DeviceHandle* h);
int dev_num_levels(const DeviceHandle* h);
int dev_layout(const DeviceHandle* h);
int dev_level_format(const DeviceHandle* h, int level);
// fp32 storage of the operators the cycle streams (mamg.h mamg_set_cycle_storage)
int dev_set_cycle_storage(DeviceHandle* h, int storage, std::string* err);
int dev_level_storage(const DeviceHandle* h, int level);
// nonlinear AMLI: the inner CG's steps inside the coarse tail (mamg.h
// mamg_set_kcycle_tail), the state, and what one apply issues (mamg_apply_launches)
int dev_set_kcycle_tail(DeviceHandle* h, int on, std::string* err);
int dev_kcycle_tail(const DeviceHandle* h);
int dev_apply_launches(const DeviceHandle* h, int64_t* launches, std::string* err);
// the coarse tail's plan (mamg_test.h mamg_tail_info)
int dev_tail_info(const DeviceHandle* h, int index, int64_t* info, int cap);
// the row-pattern dictionary's decision for level 0's A (mamg_test.h mamg_rowdict_info)
int dev_rowdict_info(const DeviceHandle* h, int64_t* info, int cap);
// the matrix-free level-0 post step's decision (mamg_test.h mamg_post_mf_info)
int dev_post_mf_info(const DeviceHandle* h, int64_t* info, int cap);
mamg_params dev_params(const DeviceHandle* h);
// the switches the handle was built with (dev_upload's sw, dev_from_ghier's G->sw)
const Switches& dev_switches(const DeviceHandle* h);
void dev_kregion(const DeviceHandle* h, std::vector<double>* ms, int* kept);
double dev_apply_bytes(const DeviceHandle* h);
int dev_apply(DeviceHandle* h, const double* d_r, double* d_z, void* stream, std::string* err);
int dev_apply_host(DeviceHandle* h, const double* r, double* z, std::string* err);
int dev_spmv(DeviceHandle* h, const double* d_x, double* d_y, void* stream, std::string* err);
int dev_pcg(DeviceHandle* h, const double* d_b, double* d_x, double tol, int maxiter,
            int relativeconv, double* residuals, double* alphas, double* betas,
            int* niters, void* stream, std::string* err);
int dev_time_apply(DeviceHandle* h, const double* d_r, double* d_z, int reps, int mode,
                   double* ms, double* kernel_ms, double* class_bytes, void* stream,
                   std::string* err);

// multi-GPU (dist_layout.hip: dist_check, dist_upload; dist_apply.hip: the rest)
struct DistHandle;
int dist_get_unique_id(void* id, std::string* err);
// ghosts: precomputed ghost lists (ghier_download_rank), else nullptr; G / A0d:
// build the rank-local operators on the device from this GPU hierarchy (H then
// holds only level sizes and the coarsest inverse)
// the multi-GPU path's parameter limits (maxit 1, no SCHWARZ_PATCHES /
// SCHWARZ_RINGS), checked before a rank touches its GPU
int dist_check(const mamg_params& p, std::string* err);
int dist_upload(const Hierarchy& H, const CsrView& A0, const mamg_params& p, const Switches& sw, int rank,
                int nranks, const void* comm_id, int64_t rep_nodes, DistHandle** out, std::string* err,
                const std::vector<std::vector<std::vector<int64_t>>>* ghosts = nullptr,
                const GHier* G = nullptr, const DevMat* A0d = nullptr);
void dist_destroy(DistHandle* h);
const Switches& dist_switches(const DistHandle* h);
void dist_range(const DistHandle* h, int64_t* o0, int64_t* o1, int64_t* nv);
// dofs per node: 2 nodal (BSR2; local vectors field-major), 1 scalar (CSR; plain slices)
int dist_dofs(const DistHandle* h);
double dist_apply_bytes(const DistHandle* h);
int dist_num_levels(const DistHandle* h);
// mamg_level_format's bits for the rank-local operators of a level
int dist_level_format(const DistHandle* h, int level);
// fp32 storage of the operators the rank's cycle streams (mamg.h
// mamg_dist_set_cycle_storage); dist_cycle_storage: MAMG_STORE_* of the handle
int dist_set_cycle_storage(DistHandle* h, int storage, std::string* err);
int dist_level_storage(const DistHandle* h, int level);
int dist_cycle_storage(const DistHandle* h);
void dist_apply_launches(const DistHandle* h, int64_t c[5]);
int dist_apply(DistHandle* h, const double* d_r, double* d_z, void* stream, std::string* err);
int dist_spmv(DistHandle* h, const double* d_x, double* d_y, void* stream, std::string* err);
int dist_virtual_spmv(const std::vector<DistHandle*>& hs, const std::vector<const double*>& x,
                      const std::vector<double*>& y, void* stream, std::string* err);
int dist_time_apply(DistHandle* h, const double* d_r, double* d_z, int reps, int mode, double* ms,
                    double* kernel_ms, double* class_bytes, void* stream, std::string* err);
int dist_set_exchange(DistHandle* h, const mamg_exchange& ex, std::string* err);
int dist_virtual_apply(const std::vector<DistHandle*>& hs, const std::vector<const double*>& r,
                       const std::vector<double*>& z, void* stream, std::string* err);
// the apply replayed from a hipGraph captured on first use per (r, z) (RCCL
// calls inside the capture); MAMG_ERR_UNSUPPORTED for host-staged / virtual
// exchanges or after a failed capture (then the eager dist_apply)
int dist_apply_graph(DistHandle* h, const double* d_r, double* d_z, void* stream, std::string* err);
// capture (or find) the graph of (r, z) without launching it
int dist_graph_prepare(DistHandle* h, const double* d_r, double* d_z, std::string* err);
int dist_virtual_apply_graph(const std::vector<DistHandle*>& hs, const std::vector<const double*>& r,
                             const std::vector<double*>& z, void* stream, std::string* err);
// device-resident PCG on the rank's local slices (dev_pcg's loop with the
// halo exchanges and the dots' all-reduces inside each iteration); stop 0:
// cbc.block's rule, 1: ||r||_2 <= tol ||b||_2 (rnorms then required)
int dist_pcg(DistHandle* h, const double* d_b, double* d_x, double tol, int maxiter, int relativeconv,
             int stop, double* residuals, double* rnorms, double* alphas, double* betas, int* niters,
             void* stream, std::string* err);
// the same on virtual ranks in lockstep; graph: one captured lockstep
// iteration replayed; every rank's state compared with rank 0's
int dist_virtual_pcg(const std::vector<DistHandle*>& hs, const std::vector<const double*>& b,
                     const std::vector<double*>& x, double tol, int maxiter, int relativeconv, int stop,
                     int graph, double* residuals, double* rnorms, double* alphas, double* betas, int* niters,
                     void* stream, std::string* err);
// what one PCG iteration issues on this rank (counts as dist_apply_launches)
void dist_pcg_launches(const DistHandle* h, int stop, int64_t c[5]);

}  // namespace mamg
