// icp.h -- what icp.hip (kernels) and api_icp.hip (host side) share: the device view of a batch of ICP jobs and the launch
// functions.  The contract is the "ICP fallback" block of include/rgbdfe.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rgbdfe {

constexpr int kIcpLeaf = 64;      // values per leaf of the reduction tree
constexpr int kIcpBlock = 256;    // source rows per workgroup of the nearest-neighbour kernel (four leaves)
constexpr int kIcpTile = 512;     // target rows staged through LDS at a time
constexpr int kIcpSums = 17;      // c, sum d2, sum P (3), sum T (3), sum T P' (9, row-major)
constexpr int kIcpScanTile = 256; // rows per tile of the valid-row compaction

// states of a job (the values of include/rgbdfe.h's RGBDFE_ICP_*)
constexpr int32_t kIcpRunning = 0, kIcpNoCorrespondences = 1, kIcpIterations = 2, kIcpTransform = 3, kIcpAbsMse = 4,
                  kIcpRelMse = 5;

// a cloud whose valid rows are compacted and sampled
struct IcpCloud {
  const float4* d;        // n rows
  uint32_t n;
  uint32_t first_tile;    // its first entry of tile_count / tile_first
  const uint32_t* pos;    // [n_samples]: positions in the ascending list of valid rows (host-computed; set before the gather)
  uint32_t n_samples;
  uint32_t poison;        // a sampled row with a non-finite x or y becomes (NaN, NaN, NaN): it then meets nothing
  float4* samples;        // [n_samples]
  uint32_t* sample_index; // [n_samples] or nullptr: the row indices
};

// a job's record, double-buffered by iteration parity: iteration k reads [(k - 1) & 1] and writes [k & 1]
struct IcpRecord {
  double mse;             // of iteration k (DBL_MAX before the first)
  float R[9], t[3];       // the increment of iteration k, R row-major
  float FR[9], Ft[3];     // F after iteration k
  int32_t done, state, k, c;
};

struct IcpJob {
  const float4* S;        // the sampled source [ns]
  const float4* T;        // the sampled target [nt]
  float4* P;              // the working copy [ns]
  int32_t ns, nt;
  int32_t* nn_j;          // [ns]: the nearest target row of the last iteration (-1: none)
  float* nn_d2;           // [ns]: its squared distance
  double* part;           // [kIcpSums][leaves]: the leaf sums, leaves = ceil(ns / 64)
  IcpRecord* rec;         // [2]
  float GR[9], Gt[3];     // the guess
};

struct IcpStop {
  double maxdist2, transformation_epsilon, euclidean_fitness_epsilon;
  int32_t max_iterations;
};

// each returns its number of kernel launches
// clouds -> tile_first (valid rows in front of every tile of 256 rows) and n_valid[cloud]; max_tiles = the largest tile
// count of a cloud
int launch_icp_compact(const IcpCloud* clouds, uint32_t n_clouds, uint32_t max_tiles, uint32_t* tile_count, uint32_t* tile_first,
                       uint32_t* n_valid, hipStream_t st);
// clouds (pos, n_samples, samples set) and tile_first -> samples; max_samples = the largest sample count of a cloud
int launch_icp_gather(const IcpCloud* clouds, uint32_t n_clouds, uint32_t max_samples, const uint32_t* tile_first,
                      hipStream_t st);
// the two kernels of iteration k, one by one (launch_icp_iterations is a loop over them)
int launch_icp_nn(const IcpJob* jobs, uint32_t n_jobs, uint32_t max_ns, IcpStop stop, int32_t k, hipStream_t st);
int launch_icp_finish(const IcpJob* jobs, uint32_t n_jobs, IcpStop stop, int32_t k, hipStream_t st);
// iterations first .. first + count - 1 of every job, each a no-op for a job that is done; max_ns = the largest ns of a job
int launch_icp_iterations(const IcpJob* jobs, uint32_t n_jobs, uint32_t max_ns, IcpStop stop, int32_t first, int32_t count,
                          hipStream_t st);

}  // namespace rgbdfe
