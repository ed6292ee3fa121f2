// Per-lesion surface distances: the twelve words of hdf_surface_distances (or _mm) for every truth lesion j against the
// predicted lesions P_j that touch it, without a full-volume pass per lesion.  Definitions: include/hdf.h.
//
//   lesion_carve_kernel   one launch for up to CHUNK lesions: both 0 / 1 byte masks of every lesion's crop, packed
//
// The crop is the box of gt_j and P_j grown by one voxel and clamped to the volume.  Every B26 seed, every C6 contour voxel
// and every 26-neighbour of a mask voxel lies inside it; a clamped side is a face of the volume ("a neighbour outside the
// volume does not exist" holds for both), an unclamped one is a layer of true background; and a mask fills the crop only if
// it fills the volume.  So the surface entry on the crop leaves the twelve words it leaves on the volume, and the host
// launches it once per lesion through its own launcher (surface.h), all on one stream and one scratch area.
//
// The crops are packed without padding, so a crop row starts at any byte: the kernel stores bytes, one a lane, 64
// consecutive ones a wave.  Integer compares and plain stores only: two calls agree in every byte.
#include "lesion_surface.h"

#include "volume_host.h"

namespace {
constexpr int CHUNK = HDF_LESION_CHUNK, BLOCK_VOX = HDF_LESION_BLOCK_VOX;
static_assert(BLOCK_VOX % 256 == 0, "whole trips of a workgroup");
typedef unsigned long long u64;

// the lesions of one launch, by value in the kernel arguments (about 2.5 KB): nothing is uploaded, nothing of the host's
// has to outlive the call
struct CarveArgs {
  int32_t n;                     // lesions in this launch
  int32_t j[CHUNK];              // truth id
  int32_t z0[CHUNK], y0[CHUNK], x0[CHUNK];
  uint32_t ch[CHUNK], cw[CHUNK];
  uint32_t cv[CHUNK];            // crop voxels (below 2^31)
  uint32_t first[CHUNK];         // the lesion's first workgroup: an exclusive scan of ceil(cv / BLOCK_VOX), first[0] = 0
  int64_t off[CHUNK];            // byte offset of the truth crop; the predicted crop is cv bytes further
};

// is the row (a, j) in the table?  rows: int64 a, b, n, m in ascending (a, b); at most 17 steps for 65536 rows
__device__ __forceinline__ bool pair_listed(const long long* __restrict__ pairs, int64_t n_pairs, int a, int j) {
  const u64 key = ((u64)(uint32_t)a << 32) | (uint32_t)j;
  int64_t lo = 0, hi = n_pairs;   // the first row with a key >= `key` is in [lo, hi]
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const u64 k = ((u64)pairs[4 * mid] << 32) | (uint32_t)pairs[4 * mid + 1];
    if (k < key) lo = mid + 1; else hi = mid;
  }
  return lo < n_pairs && pairs[4 * lo] == a && pairs[4 * lo + 1] == j;
}

// A workgroup finds its lesion by binary search over `first` and writes BLOCK_VOX consecutive bytes of each of its two
// crops; a thread's voxels are 256 apart, so a wave reads 64 consecutive voxels of a crop row (or the end of one row and
// the start of the next) from the three maps and stores 64 consecutive bytes.  Membership of a predicted id in P_j: the wave
// takes the id of its first undecided lane, looks it up once (a wave-uniform search; the last id looked up is kept, runs of
// one id are long) and decides every lane that holds it -- at most 64 rounds, usually one.
__global__ __launch_bounds__(256) void lesion_carve_kernel(const int32_t* __restrict__ ids_pred,
                                                           const int32_t* __restrict__ ids_truth,
                                                           const uint8_t* __restrict__ truth_mask, int H, int W,
                                                           const long long* __restrict__ pairs, int64_t n_pairs,
                                                           uint8_t* __restrict__ crops, const CarveArgs a) {
  int lo = 0, hi = a.n;   // first[lo] <= blockIdx.x < first[hi] (first[n]: the grid)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.first[mid] <= blockIdx.x) lo = mid; else hi = mid;
  }
  const uint32_t cv = a.cv[lo], cw = a.cw[lo], ch = a.ch[lo];
  const int j = a.j[lo], z0 = a.z0[lo], y0 = a.y0[lo], x0 = a.x0[lo];
  uint8_t* __restrict__ crop_t = crops + a.off[lo];
  uint8_t* __restrict__ crop_p = crop_t + cv;
  const uint32_t base = (blockIdx.x - a.first[lo]) * (uint32_t)BLOCK_VOX;
  int last_id = 0;          // (wave-uniform) the id looked up last, and whether (last_id, j) is a row
  bool last_hit = false;
  for (int k = 0; k < BLOCK_VOX / 256; k++) {   // (uniform: the ballots below need every lane)
    if (base + k * 256 >= cv) break;
    const uint32_t c = base + k * 256 + threadIdx.x;
    const bool in = c < cv;
    int id = 0;
    bool t = false;
    if (in) {
      const uint32_t row = c / cw, x = c - row * cw, z = row / ch, y = row - z * ch;
      const int64_t v = ((int64_t)(z0 + (int)z) * H + (y0 + (int)y)) * W + (x0 + (int)x);
      id = ids_pred[v];
      t = ids_truth[v] == j && truth_mask[v] != 0;
    }
    bool p = false, pending = id > 0;
    for (u64 todo = __ballot(pending); todo != 0; todo = __ballot(pending)) {
      const int pick = __builtin_amdgcn_readfirstlane(__shfl(id, __ffsll((long long)todo) - 1, 64));
      if (pick != last_id) last_id = pick, last_hit = pair_listed(pairs, n_pairs, pick, j);
      if (id == pick) p = last_hit, pending = false;
    }
    if (in) crop_t[c] = t ? 1 : 0, crop_p[c] = p ? 1 : 0;
  }
}
}  // namespace

int hdf_lesion_surface_plan(const char* who, const int32_t* lesions, int64_t L, int D, int H, int W, bool mm, LesionPlan* plan) {
  plan->crops.clear();
  plan->crops.reserve((size_t)L);
  const int dims[3] = {D, H, W};
  int64_t at = 0, scratch = 0;
  for (int64_t i = 0; i < L; i++) {
    const int32_t* r = lesions + 7 * i;
    HDF_CHECK_ARG(r[0] >= 1, "surface: %s: lesion row %lld: truth id %d (1 or more)", who, (long long)i, r[0]);
    int lo[3], n[3];
    for (int k = 0; k < 3; k++) {
      const int mn = r[1 + 2 * k], mx = r[2 + 2 * k];
      HDF_CHECK_ARG(mn >= 0 && mn <= mx && mx < dims[k],
                    "surface: %s: lesion row %lld: box %d..%d on axis %d of a %dx%dx%d volume", who, (long long)i, mn, mx, k, D,
                    H, W);
      lo[k] = std::max(mn - 1, 0);
      n[k] = std::min(mx + 1, dims[k] - 1) - lo[k] + 1;
    }
    const int64_t cv = (int64_t)n[0] * n[1] * n[2];
    plan->crops.push_back(LesionCrop{r[0], lo[0], lo[1], lo[2], n[0], n[1], n[2], at});
    at += 2 * cv;
    scratch = std::max(scratch, mm ? hdf_surface_mm_ws_bytes(n[0], n[1], n[2]) : hdf_surface_ws_bytes(n[0], n[1], n[2]));
  }
  plan->scratch = up256(at);
  plan->total = plan->scratch + scratch;
  return HDF_OK;
}

int hdf_launch_lesion_surface(const int32_t* ids_pred, const int32_t* ids_truth, const uint8_t* truth_mask, int H, int W,
                              const long long* pairs, int64_t n_pairs, const LesionPlan& plan, const SurfaceSpacing* sp,
                              void* ws, unsigned long long* results, hipStream_t st) {
  uint8_t* crops = (uint8_t*)ws;
  void* scratch = (char*)ws + plan.scratch;
  const int64_t L = (int64_t)plan.crops.size();
  for (int64_t i0 = 0; i0 < L; i0 += CHUNK) {
    CarveArgs a = {};
    a.n = (int32_t)std::min<int64_t>(L - i0, CHUNK);
    uint32_t blocks = 0;   // a crop has at most 2^30 voxels: 64 crops are fewer than 2^27 workgroups
    for (int k = 0; k < a.n; k++) {
      const LesionCrop& c = plan.crops[(size_t)(i0 + k)];
      a.j[k] = c.j, a.z0[k] = c.z0, a.y0[k] = c.y0, a.x0[k] = c.x0;
      a.ch[k] = (uint32_t)c.ch, a.cw[k] = (uint32_t)c.cw;
      a.cv[k] = (uint32_t)((int64_t)c.cd * c.ch * c.cw);
      a.first[k] = blocks, a.off[k] = c.off;
      blocks += (uint32_t)ceil_div64(a.cv[k], BLOCK_VOX);
    }
    hipLaunchKernelGGL(lesion_carve_kernel, dim3(blocks), dim3(256), 0, st, ids_pred, ids_truth, truth_mask, H, W, pairs,
                       n_pairs, crops, a);
    HDF_LAUNCH_CHECK();
  }
  for (int64_t i = 0; i < L; i++) {
    const LesionCrop& c = plan.crops[(size_t)i];
    const uint8_t* crop_t = crops + c.off;
    const uint8_t* crop_p = crop_t + (int64_t)c.cd * c.ch * c.cw;
    if (sp)
      HDF_TRY(hdf_launch_surface_distances_mm(crop_t, crop_p, 1, c.cd, c.ch, c.cw, *sp, scratch, results + 12 * i, st));
    else
      HDF_TRY(hdf_launch_surface_distances(crop_t, crop_p, 1, c.cd, c.ch, c.cw, scratch, results + 12 * i, nullptr, 0, st));
  }
  return HDF_OK;
}
