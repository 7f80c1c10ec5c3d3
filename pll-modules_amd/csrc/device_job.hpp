// device_job.hpp -- the host plumbing the device modules share (pll_*_dev.hip, and pll_core.hip for the allocator):
// owned device and pinned buffers, the calling thread's device put back on every path, the check of the device a
// call runs on, and DeviceJob: the device, stream, buffers and events of one call, gone when it returns.
#pragma once

#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace pllhip {

// count elements of T on the current device (0: one element); a failure leaves no sticky error behind
template <typename T>
bool dev_alloc(T ** ptr, size_t count, const char * what)
{
  const size_t bytes = (count ? count : 1) * sizeof(T);
  *ptr = nullptr;
  const hipError_t err = hipMalloc(reinterpret_cast<void **>(ptr), bytes);
  if (err == hipSuccess) return true;
  *ptr = nullptr;
  (void)hipGetLastError();
  set_error(PLL_ERROR_MEM_ALLOC, "hipMalloc of %zu bytes for %s failed: %s", bytes, what, hipGetErrorString(err));
  return false;
}

template <typename T>
bool pinned_alloc(T ** ptr, size_t count)
{
  *ptr = nullptr;
  const hipError_t err = hipHostMalloc(reinterpret_cast<void **>(ptr), count * sizeof(T));
  if (err == hipSuccess) return true;
  *ptr = nullptr;
  (void)hipGetLastError();
  set_error(PLL_ERROR_MEM_ALLOC, "hipHostMalloc of the staging buffer (%zu bytes) failed: %s", count * sizeof(T),
            hipGetErrorString(err));
  return false;
}

// one device allocation, freed with the scope unless release() has handed it on
template <typename T> struct DevBuf
{
  T * p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf & operator=(const DevBuf &) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
  bool alloc(size_t count, const char * what) { return dev_alloc(&p, count, what); }
  T * release() { T * q = p; p = nullptr; return q; }
};

// ... and one pinned host allocation
template <typename T> struct PinnedBuf
{
  T * p = nullptr;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf &) = delete;
  PinnedBuf & operator=(const PinnedBuf &) = delete;
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
  bool alloc(size_t count) { return pinned_alloc(&p, count); }
};

// the calling thread's device, put back when the scope ends
struct DeviceScope
{
  int saved = -1;
  DeviceScope() = default;
  DeviceScope(const DeviceScope &) = delete;
  DeviceScope & operator=(const DeviceScope &) = delete;
  ~DeviceScope() { if (saved >= 0) (void)hipSetDevice(saved); }
  bool save() { return hip_ok(hipGetDevice(&saved), "hipGetDevice"); }      // (the caller switches devices itself)
  bool enter(int device) { return save() && hip_ok(hipSetDevice(device), "hipSetDevice"); }
};

// the device pllhip_get_device() names, if it is visible
inline bool caller_device(const char * who, int * device)
{
  *device = pllhip_get_device();
  if (*device >= 0 && *device < pllhip_device_count()) return true;
  set_error(PLL_ERROR_HIP_NODEVICE, "%s runs on HIP device %d; %d visible", who, *device, pllhip_device_count());
  return false;
}

// the device tables of an engine's tip pointers (vectors; codes, null without coded tips), uploaded on the engine's
// stream and complete on return (pll_core.hip)
bool tip_pointer_tables(Engine * e, DevBuf<const double *> & clv, DevBuf<const uint8_t *> & codes);

// the transition matrices and the model block of the engine that executes for `p` (its own, or its first shard's, which
// gets the caller's model arrays first), as they stand once the queued matrix requests and a changed model have gone to
// the device on that engine's stream; the offsets are in doubles from `model` (pll_core.hip)
struct MatrixTables
{
  const double * pmat = nullptr;                   // [matrix][rate][S][Sp]
  const double * model = nullptr;
  unsigned off_weights = 0, off_pinv = 0, off_freqs = 0;
};
bool matrix_tables(pll_partition_t * p, MatrixTables & out);

// the per-site, per-rate likelihood table of an edge (kernels_sitecat.hpp) into the caller's rate-major planes on the
// partition's device: A[r][plane] and c[sites], B[r][plane] when it is not null; `plane` is even and the planes are
// 16-byte aligned.  Makes the operand set-up every edge reader makes (model, queued matrices, lookup tables, vectors
// and scaler counts that exist as their operation only) and enqueues the family's kernel on the engine's stream; the
// partition must not be a router (pll_core.hip)
struct SiteCatPlanes
{
  double * A = nullptr, * B = nullptr;
  unsigned * c = nullptr;
  size_t plane = 0;
};
bool sitecat_edge_table(pll_partition_t * p, unsigned parent_clv, int parent_scaler, unsigned child_clv, int child_scaler,
                        unsigned matrix_index, const unsigned * freqs_indices, const SiteCatPlanes & planes);

// the endpoint-pair table of an edge (kernels_substmap.hpp) in three steps, each enqueued on the engine's stream and
// none waited for, so that the caller can put events between them; the partition must not be a router (pll_core.hip).
// substmap_shape: what the caller has to allocate for this partition.  substmap_scale: the operand set-up of
// sitecat_edge_table, the table of the edge (and, for `differ`, the table under the matrices with a zeroed diagonal,
// which needs pm0 and lut0), then scale, differ and dropped.  substmap_pairs: the family's pair kernel into `partial`.
// substmap_reduce: F and pairs.  All buffers are the caller's, on the partition's device.
struct SubstmapShape
{
  size_t plane = 0;           // doubles per rate of the table planes (even)
  size_t splane = 0;          // doubles per rate of the scale plane (whole 32-site blocks)
  unsigned grid = 0;          // workgroups of the pair kernel = partial tiles per rate
  size_t pm_cells = 0;        // doubles of a matrix set [R][S][Sp]
  size_t lut_cells = 0;       // doubles of a lookup-table set [R][codes][S] (0: no coded tips)
  bool pinv = false;          // some category has an invariant part: the table has a B plane
};
struct SubstmapBuffers
{
  double * A = nullptr, * B = nullptr, * A0 = nullptr;       // [R][plane]; B, A0 may be null
  unsigned * c = nullptr;                                    // [N]
  unsigned * m = nullptr;                                    // [N] pattern weights
  double * scale = nullptr;                                  // [R][splane]
  double * differ = nullptr;                                 // [N] or null
  unsigned long long * dropped = nullptr;                    // 1, zeroed by substmap_scale
  double * pm0 = nullptr, * lut0 = nullptr;                  // with differ only
  double * partial = nullptr;                                // [grid][R][S][S]
  double * F = nullptr, * pairs = nullptr;                   // [R][S][S]
};
bool substmap_shape(pll_partition_t * p, const unsigned * freqs_indices, SubstmapShape & shape);
bool substmap_scale(pll_partition_t * p, unsigned parent_clv, int parent_scaler, unsigned child_clv, int child_scaler,
                    unsigned matrix_index, const unsigned * freqs_indices, const SubstmapShape & shape,
                    const SubstmapBuffers & buf);
bool substmap_pairs(pll_partition_t * p, unsigned parent_clv, unsigned child_clv, const SubstmapShape & shape,
                    const SubstmapBuffers & buf);
bool substmap_reduce(pll_partition_t * p, unsigned matrix_index, const unsigned * freqs_indices,
                     const SubstmapShape & shape, const SubstmapBuffers & buf);

// The joint sample of the ancestral states (kernels_ancsample.hpp; contract: INTEGRATION.md, "Sampled ancestral
// states"), in two steps on the engine's stream; the partition must not be a router (pll_core.hip).
// ancsample_operands: the operand set-up of a reader of all the named vectors -- model, queued matrices, tip map,
// invariant states, and every vector of `nodes` stored where it existed as its operation or as a class table only --
// and the device views of these vectors in the order of `nodes`.  Fails, naming the node, where a vector is still
// unstored afterwards.  ancsample_walk: one launch of k_ancsample_walk.
struct AncsVector
{
  const double * clv = nullptr;
  const uint8_t * codes = nullptr;             // a coded tip: its byte codes, read through the tip map
};
// one edge of the program (sim_plan.hpp, Step) as the kernel reads it
struct AncsStep
{
  AncsVector child;
  unsigned long long pm = 0;                   // doubles from the first matrix to the edge's own
  unsigned stream = 0;                         // 3 + matrix index
  unsigned src = 0, dst = 0;                   // slots (dst ~0u: the child keeps none)
  unsigned row = 0;                            // output row of the child (~0u: not asked for)
};
struct AncsOperands
{
  const double * pmat = nullptr;               // [matrix][R][S][Sp]
  const double * weights = nullptr;            // [R]
  const double * freqs = nullptr;              // [rate matrix][Sp]
  ParamIdxHost fidx = {};
  const int * invariant = nullptr;             // [sites], or null
  const unsigned long long * tipmap = nullptr;
  unsigned brows = 0;                          // state rows per blocked unit (0: the API layout)
  unsigned R = 0, S = 0, Sp = 0;
  unsigned cu_count = 0;
};
struct AncsLaunch
{
  const AncsStep * steps = nullptr;
  unsigned nsteps = 0, slots = 0;
  AncsVector root, other;
  unsigned long long pm0 = 0;                  // the root matrix, as AncsStep::pm
  unsigned root_row = 0;
  const double * A = nullptr, * B = nullptr;   // the site-category table of the root edge, [R][plane]; B may be null
  size_t plane = 0;
  const unsigned * m = nullptr;                // [sites] pattern weights
  unsigned long long * dropped = nullptr;      // null: this launch does not count
  unsigned long long seed = 0;
  unsigned first_replicate = 0;                // absolute number of replicate 0 of the launch
  unsigned replicates = 0, per_pass = 0;       // per_pass <= ANCS_RC
  unsigned site0 = 0, sites = 0, tiles = 0;    // patterns site0 .. site0 + sites - 1 are columns 0 .. sites - 1
  unsigned rows = 0, comp_row = 0;             // rows per replicate in `out`; the row of the component bytes (~0u: none)
  size_t pitch = 0;
  uint8_t * out = nullptr;                     // [replicate][rows][pitch], 0xFF before the launch
  const uint8_t * alphabet = nullptr;          // [256]
};
bool ancsample_operands(pll_partition_t * p, const unsigned * freqs_indices, const unsigned * nodes, unsigned count,
                        AncsOperands & ops, AncsVector * views);
bool ancsample_walk(pll_partition_t * p, const AncsOperands & ops, const AncsLaunch & launch, unsigned grid);

// A stage between the walk and the copy of every staging half (pll_ancsample_dev.hip, ancsample_run; used by
// pll_history_dev.hip).  The half holds [replicate][rows][pitch] bytes: state indices in the rows of all nodes, tips
// included, the component in comp_row, and extra_rows rows of the hook's own from extra_row on, 0xFF before the walk.
// prepare runs once inside the job, after the arguments passed every check and before the first launch; launch
// enqueues on the job's stream; deliver sees the pinned copy of a half; finish runs after the last delivery.
struct DeviceJob;
struct AncsStaged
{
  uint8_t * half = nullptr;                            // on the device for launch, pinned for deliver
  unsigned rep0 = 0, reps = 0, col0 = 0, cols = 0;     // replicates and patterns of the chunk
  unsigned rows = 0, comp_row = 0, extra_row = 0;
  size_t pitch = 0;
};
struct AncsStageHook
{
  unsigned flags = 0;                                  // flags of the caller's that are the hook's
  unsigned extra_rows = 0;
  unsigned long long chunk_replicates = 0;             // replicates per staging chunk, at most (0: no cap)
  virtual bool prepare(DeviceJob & j, unsigned cu_count, const unsigned * d_pattern_weights) = 0;
  virtual bool launch(DeviceJob & j, const AncsStaged & s) = 0;
  virtual void deliver(const AncsStaged & s) = 0;
  virtual bool finish(DeviceJob & j) = 0;
  virtual ~AncsStageHook() = default;
};
// times_ms (with a hook): table, walk, hook, copy
int ancsample_run(const char * who, pll_partition_t * partition, const pllhip_ancsample_params_t * params,
                  unsigned int root_node, int root_scaler, unsigned int other_node, int other_scaler,
                  unsigned int edge_count, const unsigned int * parent, const unsigned int * child,
                  const unsigned int * matrix_indices, const unsigned int * freqs_indices, unsigned int node_count,
                  unsigned char * out, unsigned char * component, unsigned long long * dropped, AncsStageHook * hook,
                  double * times_ms);

// category weights a site-category or pair table can be made under: finite, non-negative, not all zero
inline bool check_category_weights(const double * w, unsigned R, const char * who)
{
  double sum = 0.0;
  for (unsigned r = 0; r < R; ++r)
  {
    if (!(w[r] >= 0.0) || !std::isfinite(w[r]))
    {
      set_error(PLL_ERROR_PARAM_INVALID, "%s: weight %u is negative or not finite", who, r);
      return false;
    }
    sum += w[r];
  }
  if (sum > 0.0) return true;
  set_error(PLL_ERROR_PARAM_INVALID, "%s: the weights add up to 0", who);
  return false;
}

inline unsigned grid_for(size_t items, unsigned per_block)
{
  return (unsigned)std::max<size_t>(1, std::min<size_t>((items + per_block - 1) / per_block, 4096));
}

// <env>=<n>: at most n workgroups (0 or unset: no cap), read at every call -- a test knob: with a small cap a wave or a
// thread walks several strides at a size a test can afford
inline unsigned capped_grid(const char * env, unsigned long long wanted)
{
  const char * v = getenv(env);
  const long long cap = v ? atoll(v) : 0;
  if (cap > 0 && (unsigned long long)cap < wanted) wanted = (unsigned long long)cap;
  return (unsigned)std::max<unsigned long long>(1, wanted);
}

// <env>=<0..64>: only that many bits of a hash are used (a test knob: with few bits the full compare and the probing
// carry the result)
inline unsigned long long hash_keep_mask(const char * env)
{
  const char * v = getenv(env);
  if (!v || !*v) return ~0ULL;
  const long bits = std::max(0L, std::min(64L, atol(v)));
  return bits >= 64 ? ~0ULL : ((1ULL << bits) - 1ULL);
}

// everything one call owns on a device: when it goes, the stream is idle, the buffers, the pinned memory and the
// events are gone, a stream of its own is destroyed and the caller's device is current again
struct DeviceJob
{
  hipStream_t stream = nullptr;

  DeviceJob() = default;
  DeviceJob(const DeviceJob &) = delete;
  DeviceJob & operator=(const DeviceJob &) = delete;
  ~DeviceJob()
  {
    if (stream) (void)hipStreamSynchronize(stream);
    for (void * p : bufs) (void)hipFree(p);
    for (void * p : pins) (void)hipHostFree(p);
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
  }                                                             // (then `scope` puts the device back)

  // no borrowed stream: a non-blocking stream of the job's own
  bool enter(int device, hipStream_t borrowed = nullptr)
  {
    if (!scope.enter(device)) return false;
    if (borrowed) { stream = borrowed; return true; }
    own_stream = true;
    return hip_ok(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate");
  }

  // nullptr on failure
  template <typename T> T * alloc(size_t count, const char * what)
  {
    T * p = nullptr;
    if (dev_alloc(&p, count, what)) bufs.push_back(const_cast<void *>(static_cast<const void *>(p)));
    return p;
  }
  // (a buffer the result keeps)
  void keep(const void * p) { bufs.erase(std::remove(bufs.begin(), bufs.end(), p), bufs.end()); }

  template <typename T> T * pinned(size_t count)
  {
    T * p = nullptr;
    if (pinned_alloc(&p, count)) pins.push_back(p);
    return p;
  }

  hipEvent_t event(unsigned flags = hipEventDefault)
  {
    hipEvent_t e = nullptr;
    if (!hip_ok(hipEventCreateWithFlags(&e, flags), "hipEventCreate")) return nullptr;
    events.push_back(e);
    return e;
  }
  // a new event, recorded on the stream
  hipEvent_t mark()
  {
    hipEvent_t e = event();
    return e && hip_ok(hipEventRecord(e, stream), "hipEventRecord") ? e : nullptr;
  }
  bool elapsed(hipEvent_t a, hipEvent_t b, float * ms)
  {
    return hip_ok(hipEventElapsedTime(ms, a, b), "hipEventElapsedTime");
  }

  template <typename T> bool upload(T * dst, const T * src, size_t count, const char * what)
  {
    return hip_ok(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, stream), what);
  }
  template <typename T> bool download(T * dst, const T * src, size_t count, const char * what)
  {
    return hip_ok(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, stream), what);
  }

private:
  DeviceScope scope;
  bool own_stream = false;
  std::vector<void *> bufs, pins;
  std::vector<hipEvent_t> events;
};

} // namespace pllhip
