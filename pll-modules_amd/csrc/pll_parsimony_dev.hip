// pll_parsimony_dev.hip -- device side of pll_fastparsimony_* and pllhip_parsimony_tree_score (parsimony_dev.h):
// packing of the engine's tip data into bit-sliced state sets, and the walks of kernels_parsimony.hpp.
//
// A partition is one unit (its device, a stream of the object's own); a partition spread over devices by
// pllhip_set_sharding is one unit per shard.  Shards hold disjoint sites, so their counts add up exactly.
#include "device_job.hpp"
#include "kernels_parsimony.hpp"
#include "parsimony_dev.h"

#include <cstring>
#include <new>
#include <vector>

using namespace pllhip;

namespace {

struct ParsUnit
{
  int device = 0;
  hipStream_t stream = nullptr;
  unsigned nw = 0;                    // words per state (multiple of PARS_WG)
  unsigned nplanes = 0;               // weight bit planes
  uint32_t * d_sets = nullptr;        // D: [node][state][nw]
  uint32_t * d_up = nullptr;          // U: [node][state][nw] (inner nodes only are written)
  uint32_t * d_planes = nullptr;      // [nplanes][nw]
  int * d_ops = nullptr;
  unsigned long long * d_out = nullptr;   // [edges] + score
  unsigned long long * h_out = nullptr;   // pinned copy of d_out
  int * h_ops = nullptr;                  // pinned staging of the schedule
  unsigned npre = 0;                      // of the last launch
  uint32_t * d_scr = nullptr;             // SPR scratch: [member][slot][state][nw]
  unsigned spr_batch = 0;                 // members d_scr holds
  unsigned nout = 0;                      // counts of the last SPR launch
};

} // namespace

struct pllhip_pars_dev_s
{
  unsigned S = 0, tips = 0, nodes = 0;
  size_t ops_cap = 0, out_cap = 0;
  std::vector<ParsUnit> units;
};

static size_t vec_words(const pllhip_pars_dev_t * d, const ParsUnit & u) { return (size_t)d->S * u.nw; }

static void unit_free(ParsUnit & u)
{
  if (u.stream) (void)hipSetDevice(u.device);
  if (u.stream) (void)hipStreamSynchronize(u.stream);
  (void)hipFree(u.d_sets);
  (void)hipFree(u.d_up);
  (void)hipFree(u.d_planes);
  (void)hipFree(u.d_ops);
  (void)hipFree(u.d_out);
  (void)hipFree(u.d_scr);
  if (u.h_out) (void)hipHostFree(u.h_out);
  if (u.h_ops) (void)hipHostFree(u.h_ops);
  if (u.stream) (void)hipStreamDestroy(u.stream);
  u = ParsUnit();
}

// one ordinary (non-router) partition: sites [0, p->sites) of it, weights from `weights`
static bool unit_create(pllhip_pars_dev_t * d, ParsUnit & u, const pll_partition_t * p, const unsigned * weights)
{
  const Engine * e = engine_of(p);
  u.device = e->device;
  if (!hip_ok(hipSetDevice(u.device), "hipSetDevice")) return false;
  if (!hip_ok(hipStreamCreateWithFlags(&u.stream, hipStreamNonBlocking), "hipStreamCreate")) return false;
  const unsigned nreal = e->Nreal;
  const unsigned words = (nreal + 31u) / 32u;
  u.nw = std::max(1u, (words + PARS_WG - 1u) / PARS_WG) * PARS_WG;
  unsigned maxw = 0;
  for (unsigned n = 0; n < nreal; ++n) maxw = std::max(maxw, weights[n]);
  u.nplanes = 0;
  while (u.nplanes < 32 && (maxw >> u.nplanes)) ++u.nplanes;
  const size_t vec = vec_words(d, u);
  if (!dev_alloc(&u.d_sets, (size_t)d->nodes * vec, "parsimony sets") ||
      !dev_alloc(&u.d_up, (size_t)d->nodes * vec, "parsimony up-sets") ||
      !dev_alloc(&u.d_planes, (size_t)std::max(1u, u.nplanes) * u.nw, "parsimony weights") ||
      !dev_alloc(&u.d_ops, d->ops_cap, "parsimony schedule") ||
      !dev_alloc(&u.d_out, d->out_cap, "parsimony costs"))
    return false;
  if (!hip_ok(hipHostMalloc(reinterpret_cast<void **>(&u.h_out), d->out_cap * sizeof(unsigned long long)),
               "hipHostMalloc costs") ||
      !hip_ok(hipHostMalloc(reinterpret_cast<void **>(&u.h_ops), d->ops_cap * sizeof(int)), "hipHostMalloc schedule"))
    return false;

  // weights as bit planes
  std::vector<uint32_t> planes((size_t)std::max(1u, u.nplanes) * u.nw, 0u);
  for (unsigned n = 0; n < nreal; ++n)
    for (unsigned b = 0; b < u.nplanes; ++b)
      if ((weights[n] >> b) & 1u) planes[(size_t)b * u.nw + n / 32u] |= 1u << (n % 32u);
  if (!hip_ok(hipMemcpyAsync(u.d_planes, planes.data(), planes.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                              u.stream), "upload weight planes"))
    return false;

  // the tips, from the engine's device data (after whatever the engine's stream still has to upload)
  DevBuf<unsigned long long> d_tipmap;
  if (e->coded_tips &&
      (!d_tipmap.alloc(PLL_ASCII_SIZE, "parsimony code table") ||
       !hip_ok(hipMemcpyAsync(d_tipmap.p, p->tipmap, PLL_ASCII_SIZE * sizeof(unsigned long long), hipMemcpyHostToDevice,
                              u.stream), "upload code table")))
    return false;
  bool ok = hip_ok(hipStreamSynchronize(e->stream), "engine stream");
  for (unsigned t = 0; ok && t < d->tips; ++t)
  {
    const bool coded = e->coded_tips;
    hipLaunchKernelGGL(k_pars_pack, dim3(u.nw / 2u), dim3(PARS_WG), 0, u.stream,
                       coded ? nullptr : e->d_clv[t], coded ? e->d_codes[t] : nullptr, d_tipmap.p,
                       e->blocked ? 1u : 0u, e->R, e->Sp, e->rows, d->S, nreal, u.nw, u.d_sets + (size_t)t * vec);
    ok = hip_ok(hipGetLastError(), "k_pars_pack");
  }
  return ok && hip_ok(hipStreamSynchronize(u.stream), "pack tips");
}

extern "C" pllhip_pars_dev_t * pllhip_pars_dev_create(const pll_partition_t * p)
{
  const Engine * e = engine_of(p);
  if (!e)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "The partition has no engine state");
    return nullptr;
  }
  if (p->states < 2 || p->states > 64)
  {
    set_error(PLL_ERROR_STEPWISE_UNSUPPORTED, "Parsimony takes 2 .. 64 states, not %u", p->states);
    return nullptr;
  }
  pllhip_pars_dev_t * d = new (std::nothrow) pllhip_pars_dev_t();
  if (!d)
  {
    set_error(PLL_ERROR_MEM_ALLOC, "Cannot allocate parsimony state");
    return nullptr;
  }
  DeviceScope scope;
  (void)scope.save();
  d->S = p->states;
  d->tips = p->tips;
  d->nodes = std::max(p->tips, 2u * p->tips - 2u);
  d->ops_cap = 3u * (size_t)d->nodes + 4u * (size_t)d->nodes + 8u;
  d->out_cap = (size_t)d->nodes + 1u;
  bool ok = true;
  if (e->shards.empty())
  {
    d->units.emplace_back();
    ok = unit_create(d, d->units.back(), p, p->pattern_weights);
  }
  else
    for (size_t k = 0; ok && k < e->shards.size(); ++k)
    {
      d->units.emplace_back();
      ok = unit_create(d, d->units.back(), e->shards[k], p->pattern_weights + e->shard_first[k]);
    }
  if (!ok)
  {
    pllhip_pars_dev_destroy(d);
    return nullptr;
  }
  return d;
}

extern "C" void pllhip_pars_dev_destroy(pllhip_pars_dev_t * d)
{
  if (!d) return;
  DeviceScope scope;
  (void)scope.save();
  for (ParsUnit & u : d->units) unit_free(u);
  delete d;
}

extern "C" int pllhip_pars_dev_launch(pllhip_pars_dev_t * d, const int * ops, unsigned ndown, unsigned npre, int cand,
                                      int count_score)
{
  const size_t nops = 3u * (size_t)ndown + 4u * (size_t)npre;
  if (nops > d->ops_cap || npre + 1u > d->out_cap || (npre && (cand < 0 || (unsigned)cand >= d->nodes)))
  {
    set_error(PLL_ERROR_PARAM_INVALID, "Parsimony schedule out of range");
    return PLL_FAILURE;
  }
  for (size_t i = 0; i < nops; ++i)
    if (ops[i] >= (int)d->nodes)
    {
      set_error(PLL_ERROR_PARAM_INVALID, "Parsimony schedule names node %d of %u", ops[i], d->nodes);
      return PLL_FAILURE;
    }
  DeviceScope scope;
  (void)scope.save();
  for (ParsUnit & u : d->units)
  {
    PLLHIP_TRY(hipSetDevice(u.device));
    PLLHIP_TRY(hipStreamSynchronize(u.stream));             // h_ops / h_out are free again
    memcpy(u.h_ops, ops, nops * sizeof(int));
    const size_t vec = vec_words(d, u);
    PLLHIP_TRY(hipMemsetAsync(u.d_out, 0, (npre + 1u) * sizeof(unsigned long long), u.stream));
    PLLHIP_TRY(hipMemcpyAsync(u.d_ops, u.h_ops, std::max<size_t>(1, nops) * sizeof(int), hipMemcpyHostToDevice,
                              u.stream));
    hipLaunchKernelGGL(k_pars_walk, dim3(u.nw / PARS_WG), dim3(PARS_WG), 0, u.stream, u.d_sets, u.d_up, vec, d->S,
                       u.nw, (const uint32_t *)u.d_planes, u.nplanes, (const int *)u.d_ops, ndown, npre,
                       (const uint32_t *)(u.d_sets + (size_t)(cand < 0 ? 0 : cand) * vec), u.d_out,
                       count_score ? u.d_out + npre : nullptr);
    PLLHIP_TRY(hipGetLastError());
    PLLHIP_TRY(hipMemcpyAsync(u.h_out, u.d_out, (npre + 1u) * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                              u.stream));
    u.npre = npre;
  }
  return PLL_SUCCESS;
}

extern "C" int pllhip_pars_dev_collect(pllhip_pars_dev_t * d, unsigned long long * edge_acc,
                                       unsigned long long * score_acc)
{
  DeviceScope scope;
  (void)scope.save();
  for (ParsUnit & u : d->units)
  {
    PLLHIP_TRY(hipSetDevice(u.device));
    PLLHIP_TRY(hipStreamSynchronize(u.stream));
    if (edge_acc)
      for (unsigned i = 0; i < u.npre; ++i) edge_acc[i] += u.h_out[i];
    if (score_acc) *score_acc += u.h_out[u.npre];
  }
  return PLL_SUCCESS;
}

// ---------------------------------------------------------------------------------------------------------------
// SPR rounds: k_pars_spr
// ---------------------------------------------------------------------------------------------------------------

// (re)allocates the schedule and cost buffers of one unit for ops_cap / out_cap
static bool unit_grow_io(pllhip_pars_dev_t * d, ParsUnit & u)
{
  (void)hipFree(u.d_ops);
  (void)hipFree(u.d_out);
  if (u.h_out) (void)hipHostFree(u.h_out);
  if (u.h_ops) (void)hipHostFree(u.h_ops);
  u.d_ops = nullptr; u.d_out = nullptr; u.h_out = nullptr; u.h_ops = nullptr;
  return dev_alloc(&u.d_ops, d->ops_cap, "parsimony schedule") &&
         dev_alloc(&u.d_out, d->out_cap, "parsimony costs") &&
         hip_ok(hipHostMalloc(reinterpret_cast<void **>(&u.h_out), d->out_cap * sizeof(unsigned long long)),
                "hipHostMalloc costs") &&
         hip_ok(hipHostMalloc(reinterpret_cast<void **>(&u.h_ops), d->ops_cap * sizeof(int)), "hipHostMalloc schedule");
}

extern "C" unsigned pllhip_pars_dev_spr_hint(const pllhip_pars_dev_t * d)
{
  // about 2048 one-wave workgroups per launch: a few per SIMD of the chip
  const unsigned blocks = d->units[0].nw / PARS_WG;
  return std::min(PARS_SPR_MAX_BATCH, std::max(1u, (2048u + blocks - 1u) / blocks));
}

extern "C" unsigned pllhip_pars_dev_spr_reserve(pllhip_pars_dev_t * d, unsigned want)
{
  want = std::max(1u, std::min(want, PARS_SPR_MAX_BATCH));
  DeviceScope scope;
  (void)scope.save();
  unsigned batch = want;
  bool ok = true;
  for (ParsUnit & u : d->units)
  {
    if (u.spr_batch >= want) { batch = std::min(batch, u.spr_batch); continue; }
    ok = hip_ok(hipSetDevice(u.device), "hipSetDevice") && hip_ok(hipStreamSynchronize(u.stream), "parsimony stream");
    if (!ok) break;
    const size_t member_bytes = (size_t)d->nodes * vec_words(d, u) * sizeof(uint32_t);
    size_t free_b = 0, total_b = 0;
    unsigned b = want;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)           // at most a quarter of what is free
      b = (unsigned)std::max<size_t>(1, std::min<size_t>(want, free_b / 4u / member_bytes));
    (void)hipFree(u.d_scr);
    u.d_scr = nullptr;
    u.spr_batch = 0;
    ok = dev_alloc(&u.d_scr, (size_t)b * d->nodes * vec_words(d, u), "parsimony SPR scratch");
    if (!ok) break;
    u.spr_batch = b;
    batch = std::min(batch, b);
  }
  // schedules and costs of `batch` members, each at most one path and one edge op per node
  const size_t ops_need = (size_t)batch * (PARS_MEMBER_INTS + (size_t)d->nodes * (PARS_SPR_DOWN_INTS + PARS_SPR_PRE_INTS));
  const size_t out_need = (size_t)batch * d->nodes;
  if (ok && (ops_need > d->ops_cap || out_need > d->out_cap))
  {
    d->ops_cap = std::max(d->ops_cap, ops_need);
    d->out_cap = std::max(d->out_cap, out_need);
    for (ParsUnit & u : d->units)
    {
      ok = hip_ok(hipSetDevice(u.device), "hipSetDevice") && hip_ok(hipStreamSynchronize(u.stream), "stream") &&
           unit_grow_io(d, u);
      if (!ok) break;
    }
  }
  return ok ? batch : 0u;
}

static bool spr_operand_ok(int o, unsigned nodes)
{
  if (o < 0) return false;
  const unsigned src = (unsigned)o & 3u;
  return src <= PARS_SRC_X && ((unsigned)o >> 2) < nodes;       // node ids and scratch slots are both < nodes
}

extern "C" int pllhip_pars_dev_spr_launch(pllhip_pars_dev_t * d, const int * ops, size_t nops, const int * members,
                                          unsigned nmem, unsigned nout)
{
  const size_t nint = nops + (size_t)PARS_MEMBER_INTS * nmem;
  bool ok = nmem > 0 && nint <= d->ops_cap && nout <= d->out_cap;
  for (ParsUnit & u : d->units) ok = ok && nmem <= u.spr_batch;
  for (unsigned m = 0; ok && m < nmem; ++m)
  {
    const int * mem = members + PARS_MEMBER_INTS * m;
    const int first = mem[0], ndown = mem[1], npre = mem[2], cand = mem[3], out0 = mem[4];
    ok = first >= 0 && ndown >= 0 && npre >= 0 && cand >= 0 && (unsigned)cand < d->nodes && out0 >= 0 &&
         (size_t)first + (size_t)ndown * PARS_SPR_DOWN_INTS + (size_t)npre * PARS_SPR_PRE_INTS <= nops;
    const int * op = ops + (ok ? first : 0);
    for (int k = 0; ok && k < ndown; ++k, op += PARS_SPR_DOWN_INTS)
      ok = op[0] >= 0 && (unsigned)op[0] < d->nodes && spr_operand_ok(op[1], d->nodes) &&
           spr_operand_ok(op[2], d->nodes);
    unsigned counted = 0;
    for (int e = 0; ok && e < npre; ++e, op += PARS_SPR_PRE_INTS)
    {
      ok = spr_operand_ok(op[0], d->nodes) && spr_operand_ok(op[1], d->nodes) &&
           (op[2] < 0 || spr_operand_ok(op[2], d->nodes)) && (op[3] < 0 || (unsigned)op[3] < d->nodes);
      counted += op[4] ? 1u : 0u;
    }
    ok = ok && (size_t)out0 + counted <= nout;
  }
  if (!ok)
  {
    set_error(PLL_ERROR_PARAM_INVALID, "Parsimony SPR schedule out of range");
    return PLL_FAILURE;
  }
  DeviceScope scope;
  (void)scope.save();
  for (ParsUnit & u : d->units)
  {
    PLLHIP_TRY(hipSetDevice(u.device));
    PLLHIP_TRY(hipStreamSynchronize(u.stream));
    memcpy(u.h_ops, ops, nops * sizeof(int));
    memcpy(u.h_ops + nops, members, (size_t)PARS_MEMBER_INTS * nmem * sizeof(int));
    const size_t vec = vec_words(d, u);
    PLLHIP_TRY(hipMemsetAsync(u.d_out, 0, std::max(1u, nout) * sizeof(unsigned long long), u.stream));
    PLLHIP_TRY(hipMemcpyAsync(u.d_ops, u.h_ops, nint * sizeof(int), hipMemcpyHostToDevice, u.stream));
    hipLaunchKernelGGL(k_pars_spr, dim3(u.nw / PARS_WG, nmem), dim3(PARS_WG), 0, u.stream,
                       (const uint32_t *)u.d_sets, (const uint32_t *)u.d_up, u.d_scr, (size_t)d->nodes * vec, vec,
                       d->S, u.nw, (const uint32_t *)u.d_planes, u.nplanes, (const int *)u.d_ops,
                       (const int *)(u.d_ops + nops), u.d_out);
    PLLHIP_TRY(hipGetLastError());
    PLLHIP_TRY(hipMemcpyAsync(u.h_out, u.d_out, std::max(1u, nout) * sizeof(unsigned long long),
                              hipMemcpyDeviceToHost, u.stream));
    u.nout = nout;
  }
  return PLL_SUCCESS;
}

extern "C" int pllhip_pars_dev_spr_collect(pllhip_pars_dev_t * d, unsigned long long * acc)
{
  DeviceScope scope;
  (void)scope.save();
  for (ParsUnit & u : d->units)
  {
    PLLHIP_TRY(hipSetDevice(u.device));
    PLLHIP_TRY(hipStreamSynchronize(u.stream));
    for (unsigned i = 0; i < u.nout; ++i) acc[i] += u.h_out[i];
  }
  return PLL_SUCCESS;
}
