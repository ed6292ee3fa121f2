// The C ABI of the entries on a uint8 / int32 volume [D][H][W]: surface distances and the average surface distance, in
// voxels and in physical units (surface.hip, surface_asd.hip, surface_mm.hip), connected components (components.hip), the
// overlap table of two id maps (cc_pairs.hip), per-lesion surface distances on crops (lesion_surface.hip), binary
// morphology (morphology.hip), lesion candidates from a probability map (detect.hip), the measurements of an image
// under an id map (measure.hip) and its order statistics (quantiles.hip).  Every entry checks its arguments on
// the host -- the first check that fails decides the message, "<family>: <entry>: ..." -- and hands on to the unit's
// launcher.  Nothing here touches a plan.
#include <cmath>

#include "../../include/hdf.h"
#include "cc_pairs.h"
#include "components.h"
#include "detect.h"
#include "lesion_surface.h"
#include "measure.h"
#include "morphology.h"
#include "quantiles.h"
#include "surface.h"

namespace {
const char SURF[] = "surface", CC[] = "components", MORPH[] = "morphology", DET[] = "detect";

int check_label(const char* prefix, const char* who, int label, int lo) {
  HDF_CHECK_ARG(label >= lo && label <= 255, "%s: %s: label %d (%d..255)", prefix, who, label, lo);
  return HDF_OK;
}
int check_nonnull(const char* prefix, const char* who, bool all) {
  HDF_CHECK_ARG(all, "%s: %s: null argument", prefix, who);
  return HDF_OK;
}
int check_ws_bytes(const char* prefix, const char* who, int64_t bytes, int64_t need) {
  HDF_CHECK_ARG(bytes >= need, "%s: %s: workspace of %lld bytes, %lld needed", prefix, who, (long long)bytes, (long long)need);
  return HDF_OK;
}
int check_aligned8(const char* prefix, const char* who, const char* what, const void* p) {
  HDF_CHECK_ARG((reinterpret_cast<uintptr_t>(p) & 7) == 0, "%s: %s: %s not aligned to 8 bytes", prefix, who, what);
  return HDF_OK;
}
// a workspace in the order the component, pair and morphology entries check it: there, of the right size, aligned.  (The
// surface entries check the size first and the pointers together afterwards: they use the pieces.)
int check_workspace(const char* prefix, const char* who, const void* ws, int64_t bytes, int64_t need) {
  HDF_TRY(check_nonnull(prefix, who, ws != nullptr));
  HDF_TRY(check_ws_bytes(prefix, who, bytes, need));
  return check_aligned8(prefix, who, "workspace", ws);
}
// text: the whole complaint, e.g. "ids overlaps volume"
int check_disjoint(const char* prefix, const char* who, const void* a, int64_t na, const void* b, int64_t nb, const char* text) {
  HDF_CHECK_ARG(!hdf_overlap(a, na, b, nb), "%s: %s: %s", prefix, who, text);
  return HDF_OK;
}
int64_t ws_bytes_or_minus1(const char* prefix, const char* who, int D, int H, int W, int64_t (*size)(int, int, int)) {
  return hdf_vol_check_dims(prefix, who, D, H, W) == HDF_OK ? size(D, H, W) : -1;
}

// what the two morphology entries share
int morph_check_buffers(const char* who, const uint8_t* volume, const uint8_t* out, const uint64_t* result,
                        const void* workspace, int64_t workspace_bytes, int64_t need, int64_t V) {
  HDF_TRY(check_nonnull(MORPH, who, volume && out && result));
  HDF_TRY(check_workspace(MORPH, who, workspace, workspace_bytes, need));
  if (out != volume) HDF_TRY(check_disjoint(MORPH, who, out, V, volume, V, "out overlaps volume without being volume"));
  const char* ws_text = "workspace overlaps volume, out or result";
  HDF_TRY(check_disjoint(MORPH, who, workspace, need, volume, V, ws_text));
  HDF_TRY(check_disjoint(MORPH, who, workspace, need, out, V, ws_text));
  HDF_TRY(check_disjoint(MORPH, who, workspace, need, result, 16, ws_text));
  HDF_TRY(check_disjoint(MORPH, who, result, 16, volume, V, "result overlaps volume or out"));
  return check_disjoint(MORPH, who, result, 16, out, V, "result overlaps volume or out");
}
}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------------- surface distances, in voxels
int64_t hdf_surface_workspace_bytes(int D, int H, int W) {
  return ws_bytes_or_minus1(SURF, "workspace_bytes", D, H, W, hdf_surface_ws_bytes);
}
int hdf_op_mask_flags(const uint8_t* target, const uint8_t* prediction, int label, int D, int H, int W, uint8_t* flags,
                      uint64_t* counts, hdf_stream stream) {
  HDF_TRY(hdf_vol_check_dims(SURF, "mask_flags", D, H, W));
  HDF_TRY(check_label(SURF, "mask_flags", label, 1));
  HDF_TRY(check_nonnull(SURF, "mask_flags", target && prediction && flags && counts));
  return hdf_launch_mask_flags(target, prediction, label, D, H, W, flags, (unsigned long long*)counts, false,
                               (hipStream_t)stream);
}
int hdf_op_edt_sq(const uint8_t* flags, int seed_bit, int D, int H, int W, int32_t* d2, void* workspace,
                  int64_t workspace_bytes, hdf_stream stream) {
  HDF_TRY(hdf_vol_check_dims(SURF, "edt_sq", D, H, W));
  HDF_CHECK_ARG(seed_bit >= 1 && seed_bit <= 255, "surface: edt_sq: seed mask %d (1..255)", seed_bit);
  HDF_TRY(check_ws_bytes(SURF, "edt_sq", workspace_bytes, hdf_surface_ws_bytes(D, H, W)));
  HDF_TRY(check_nonnull(SURF, "edt_sq", flags && d2 && workspace));
  return hdf_launch_edt_sq(flags, seed_bit, D, H, W, d2, (hipStream_t)stream);
}
int hdf_surface_distances(const uint8_t* target, const uint8_t* prediction, int label, int D, int H, int W,
                          void* workspace, int64_t workspace_bytes, uint64_t* result, uint32_t* histogram_out,
                          int64_t histogram_len, hdf_stream stream) {
  HDF_TRY(hdf_vol_check_dims(SURF, "distances", D, H, W));
  HDF_TRY(check_label(SURF, "distances", label, 1));
  HDF_TRY(check_ws_bytes(SURF, "distances", workspace_bytes, hdf_surface_ws_bytes(D, H, W)));
  HDF_CHECK_ARG(histogram_len >= 0, "surface: distances: histogram_len %lld", (long long)histogram_len);
  HDF_TRY(check_nonnull(SURF, "distances", target && prediction && workspace && result));
  return hdf_launch_surface_distances(target, prediction, label, D, H, W, workspace, (unsigned long long*)result,
                                      histogram_out, histogram_len, (hipStream_t)stream);
}
int64_t hdf_surface_asd_workspace_bytes(int D, int H, int W) {
  return ws_bytes_or_minus1(SURF, "asd_workspace_bytes", D, H, W, hdf_surface_asd_ws_bytes);
}
int hdf_op_edge_flags(const uint8_t* target, const uint8_t* prediction, int label, int D, int H, int W, uint8_t* flags,
                      uint64_t* counts, hdf_stream stream) {
  HDF_TRY(hdf_vol_check_dims(SURF, "edge_flags", D, H, W));
  HDF_TRY(check_label(SURF, "edge_flags", label, 1));
  HDF_TRY(check_nonnull(SURF, "edge_flags", target && prediction && flags && counts));
  return hdf_launch_edge_flags(target, prediction, label, D, H, W, flags, (unsigned long long*)counts, false,
                               (hipStream_t)stream);
}
int hdf_surface_asd(const uint8_t* target, const uint8_t* prediction, int label, int D, int H, int W, void* workspace,
                    int64_t workspace_bytes, uint64_t* result, uint32_t* histogram_out, int64_t histogram_len,
                    hdf_stream stream) {
  HDF_TRY(hdf_vol_check_dims(SURF, "asd", D, H, W));
  HDF_TRY(check_label(SURF, "asd", label, 1));
  HDF_TRY(check_ws_bytes(SURF, "asd", workspace_bytes, hdf_surface_asd_ws_bytes(D, H, W)));
  HDF_CHECK_ARG(histogram_len >= 0, "surface: asd: histogram_len %lld", (long long)histogram_len);
  HDF_TRY(check_nonnull(SURF, "asd", target && prediction && workspace && result));
  return hdf_launch_surface_asd(target, prediction, label, D, H, W, workspace, (unsigned long long*)result, histogram_out,
                                histogram_len, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------- the same in physical units
// The spacing is a host pointer: checked, and read, before anything else.
int64_t hdf_surface_mm_workspace_bytes(int D, int H, int W) {
  return ws_bytes_or_minus1(SURF, "mm_workspace_bytes", D, H, W, hdf_surface_mm_ws_bytes);
}
int hdf_op_edt_sq_mm(const uint8_t* flags, int seed_bit, int D, int H, int W, const double* spacing, double* d2,
                     void* workspace, int64_t workspace_bytes, hdf_stream stream) {
  SurfaceSpacing sp;
  HDF_TRY(hdf_surface_check_spacing("edt_sq_mm", spacing, &sp));
  HDF_TRY(hdf_vol_check_dims(SURF, "edt_sq_mm", D, H, W));
  HDF_CHECK_ARG(seed_bit >= 1 && seed_bit <= 255, "surface: edt_sq_mm: seed mask %d (1..255)", seed_bit);
  HDF_TRY(check_ws_bytes(SURF, "edt_sq_mm", workspace_bytes, hdf_surface_mm_ws_bytes(D, H, W)));
  HDF_TRY(check_nonnull(SURF, "edt_sq_mm", flags && d2 && workspace));
  HDF_TRY(check_aligned8(SURF, "edt_sq_mm", "d2", d2));
  return hdf_launch_edt_sq_mm(flags, seed_bit, D, H, W, sp, d2, (hipStream_t)stream);
}
int hdf_op_select_u64(const uint64_t* keys, int64_t n, int64_t lo, void* workspace, int64_t workspace_bytes,
                      uint64_t* out2, hdf_stream stream) {
  HDF_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31), "surface: select_u64: n=%lld outside [1, 2^31)", (long long)n);
  HDF_CHECK_ARG(lo >= 0 && lo < n, "surface: select_u64: lo=%lld outside [0, n=%lld)", (long long)lo, (long long)n);
  HDF_TRY(check_ws_bytes(SURF, "select_u64", workspace_bytes, HDF_SELECT_U64_WS));
  HDF_TRY(check_nonnull(SURF, "select_u64", keys && workspace && out2));
  HDF_TRY(check_aligned8(SURF, "select_u64", "workspace", workspace));
  return hdf_launch_select_u64((const unsigned long long*)keys, n, lo, workspace, (unsigned long long*)out2,
                               (hipStream_t)stream);
}
int hdf_surface_distances_mm(const uint8_t* target, const uint8_t* prediction, int label, int D, int H, int W,
                             const double* spacing, void* workspace, int64_t workspace_bytes, uint64_t* result,
                             hdf_stream stream) {
  SurfaceSpacing sp;
  HDF_TRY(hdf_surface_check_spacing("distances_mm", spacing, &sp));
  HDF_TRY(hdf_vol_check_dims(SURF, "distances_mm", D, H, W));
  HDF_TRY(check_label(SURF, "distances_mm", label, 1));
  HDF_TRY(check_ws_bytes(SURF, "distances_mm", workspace_bytes, hdf_surface_mm_ws_bytes(D, H, W)));
  HDF_TRY(check_nonnull(SURF, "distances_mm", target && prediction && workspace && result));
  HDF_TRY(check_aligned8(SURF, "distances_mm", "workspace", workspace));
  return hdf_launch_surface_distances_mm(target, prediction, label, D, H, W, sp, workspace, (unsigned long long*)result,
                                         (hipStream_t)stream);
}
int hdf_surface_asd_mm(const uint8_t* target, const uint8_t* prediction, int label, int D, int H, int W,
                       const double* spacing, void* workspace, int64_t workspace_bytes, uint64_t* result,
                       hdf_stream stream) {
  SurfaceSpacing sp;
  HDF_TRY(hdf_surface_check_spacing("asd_mm", spacing, &sp));
  HDF_TRY(hdf_vol_check_dims(SURF, "asd_mm", D, H, W));
  HDF_TRY(check_label(SURF, "asd_mm", label, 1));
  HDF_TRY(check_ws_bytes(SURF, "asd_mm", workspace_bytes, hdf_surface_mm_ws_bytes(D, H, W)));
  HDF_TRY(check_nonnull(SURF, "asd_mm", target && prediction && workspace && result));
  HDF_TRY(check_aligned8(SURF, "asd_mm", "workspace", workspace));
  return hdf_launch_surface_asd_mm(target, prediction, label, D, H, W, sp, workspace, (unsigned long long*)result,
                                   (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------- connected components
int64_t hdf_cc_workspace_bytes(int D, int H, int W) {
  return ws_bytes_or_minus1(CC, "workspace_bytes", D, H, W, hdf_cc_ws_bytes);
}
int hdf_cc_label(const uint8_t* volume, int label, int connectivity, int D, int H, int W, int32_t* ids, uint64_t* result,
                 void* workspace, int64_t workspace_bytes, hdf_stream stream) {
  HDF_TRY(hdf_vol_check_dims(CC, "label", D, H, W));
  HDF_CHECK_ARG(connectivity == 6 || connectivity == 18 || connectivity == 26, "components: label: connectivity %d (6, 18 or 26)",
                connectivity);
  HDF_TRY(check_label(CC, "label", label, 0));
  HDF_TRY(check_nonnull(CC, "label", volume && ids && result));
  HDF_TRY(check_workspace(CC, "label", workspace, workspace_bytes, hdf_cc_ws_bytes(D, H, W)));
  const int64_t V = (int64_t)D * H * W;
  HDF_TRY(check_disjoint(CC, "label", volume, V, ids, V * 4, "ids overlaps volume"));
  return hdf_launch_cc_label(volume, label, connectivity, D, H, W, ids, (unsigned long long*)result, workspace,
                             (hipStream_t)stream);
}
int hdf_cc_table(const uint8_t* volume, const int32_t* ids, const float* score, int D, int H, int W, int64_t capacity,
                 int64_t* table, float* score_max, hdf_stream stream) {
  HDF_TRY(hdf_vol_check_dims(CC, "table", D, H, W));
  HDF_CHECK_ARG(capacity >= 1 && capacity < ((int64_t)1 << 31), "components: table: capacity %lld (1..2^31-1)",
                (long long)capacity);
  HDF_TRY(check_nonnull(CC, "table", volume && ids && table && (!score || score_max)));
  const int64_t V = (int64_t)D * H * W;
  HDF_TRY(check_disjoint(CC, "table", volume, V, ids, V * 4, "ids overlaps volume"));
  return hdf_launch_cc_table(volume, ids, score, D, H, W, capacity, (long long*)table, score_max, (hipStream_t)stream);
}
int hdf_cc_filter(const uint8_t* volume, const int32_t* ids, int D, int H, int W, int64_t min_size, int keep_largest,
                  uint8_t* out, uint64_t* result, void* workspace, int64_t workspace_bytes, hdf_stream stream) {
  HDF_TRY(hdf_vol_check_dims(CC, "filter", D, H, W));
  HDF_CHECK_ARG(min_size >= 0, "components: filter: min_size %lld is negative", (long long)min_size);
  HDF_TRY(check_nonnull(CC, "filter", volume && ids && out && result));
  HDF_TRY(check_workspace(CC, "filter", workspace, workspace_bytes, hdf_cc_ws_bytes(D, H, W)));
  const int64_t V = (int64_t)D * H * W;
  HDF_TRY(check_disjoint(CC, "filter", volume, V, ids, V * 4, "ids overlaps volume or out"));
  HDF_TRY(check_disjoint(CC, "filter", out, V, ids, V * 4, "ids overlaps volume or out"));
  if (out != volume) HDF_TRY(check_disjoint(CC, "filter", out, V, volume, V, "out overlaps volume without being volume"));
  return hdf_launch_cc_filter(volume, ids, D, H, W, min_size, keep_largest, out, (unsigned long long*)result, workspace,
                              (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------- the overlap table of two id maps
int64_t hdf_cc_pairs_workspace_bytes(int64_t capacity) {
  if (capacity < 1 || capacity > HDF_PAIRS_MAX_CAPACITY) {
    hdf_set_error("components: pairs: capacity %lld (1..%lld)", (long long)capacity, (long long)HDF_PAIRS_MAX_CAPACITY);
    return -1;
  }
  return hdf_cc_pairs_ws_bytes(capacity);
}
int hdf_cc_pairs(const int32_t* ids_a, const int32_t* ids_b, const uint8_t* mask, int flags, int D, int H, int W,
                 int64_t capacity, int64_t* pairs, uint64_t* result, void* workspace, int64_t workspace_bytes,
                 hdf_stream stream) {
  HDF_TRY(hdf_vol_check_dims(CC, "pairs", D, H, W));
  HDF_CHECK_ARG(capacity >= 1 && capacity <= HDF_PAIRS_MAX_CAPACITY, "components: pairs: capacity %lld (1..%lld)",
                (long long)capacity, (long long)HDF_PAIRS_MAX_CAPACITY);
  HDF_CHECK_ARG((flags & ~(HDF_PAIRS_A0 | HDF_PAIRS_B0)) == 0, "components: pairs: flags %d (HDF_PAIRS_A0 | HDF_PAIRS_B0)", flags);
  HDF_TRY(check_nonnull(CC, "pairs", ids_a && ids_b && pairs && result));
  const int64_t need = hdf_cc_pairs_ws_bytes(capacity), V = (int64_t)D * H * W, rows = capacity * 32;
  HDF_TRY(check_workspace(CC, "pairs", workspace, workspace_bytes, need));
  const struct { const void* p; int64_t n; const char* name; } out[3] = {{pairs, rows, "pairs"}, {result, 32, "result"},
                                                                        {workspace, need, "workspace"}};
  for (int i = 0; i < 3; i++) {
    HDF_CHECK_ARG(!hdf_overlap(out[i].p, out[i].n, ids_a, V * 4) && !hdf_overlap(out[i].p, out[i].n, ids_b, V * 4) &&
                      !(mask && hdf_overlap(out[i].p, out[i].n, mask, V)),
                  "components: pairs: %s overlaps an input", out[i].name);
    for (int j = i + 1; j < 3; j++)
      HDF_CHECK_ARG(!hdf_overlap(out[i].p, out[i].n, out[j].p, out[j].n), "components: pairs: %s overlaps %s", out[i].name,
                    out[j].name);
  }
  return hdf_launch_cc_pairs(ids_a, ids_b, mask, flags, D, H, W, capacity, (long long*)pairs, (unsigned long long*)result,
                             workspace, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------- measurements under an id map
int64_t hdf_cc_measure_workspace_bytes(int C, int64_t capacity) {
  if (C < 1 || C > HDF_MEASURE_MAX_CHANNELS || capacity < 1 || capacity > HDF_MEASURE_MAX_CAPACITY) {
    hdf_set_error("components: measure: C = %d (1..%d), capacity %lld (1..%lld)", C, HDF_MEASURE_MAX_CHANNELS,
                  (long long)capacity, (long long)HDF_MEASURE_MAX_CAPACITY);
    return -1;
  }
  return hdf_cc_measure_ws_bytes(C, capacity);
}
int hdf_cc_measure(const int32_t* ids, const float* image, int C, int D, int H, int W, int64_t capacity, int64_t* geom,
                   double* stats, int64_t* pos, uint64_t* result, void* workspace, int64_t workspace_bytes, hdf_stream stream) {
  const char* who = "measure";
  HDF_CHECK_ARG(C >= 1 && C <= HDF_MEASURE_MAX_CHANNELS, "components: %s: C = %d (1..%d)", who, C, HDF_MEASURE_MAX_CHANNELS);
  HDF_TRY(hdf_vol_check_dims(CC, who, D, H, W));
  HDF_CHECK_ARG(capacity >= 1 && capacity <= HDF_MEASURE_MAX_CAPACITY, "components: %s: capacity %lld (1..%lld)", who,
                (long long)capacity, (long long)HDF_MEASURE_MAX_CAPACITY);
  HDF_TRY(check_nonnull(CC, who, ids && image && geom && stats && pos && result));
  const int64_t need = hdf_cc_measure_ws_bytes(C, capacity), V = (int64_t)D * H * W;
  HDF_TRY(check_workspace(CC, who, workspace, workspace_bytes, need));
  HDF_TRY(check_aligned8(CC, who, "geom", geom));
  HDF_TRY(check_aligned8(CC, who, "stats", stats));
  HDF_TRY(check_aligned8(CC, who, "pos", pos));
  HDF_TRY(check_aligned8(CC, who, "result", result));
  const struct { const void* p; int64_t n; const char* name; } out[5] = {{geom, capacity * 32, "geom"},
                                                                        {stats, C * capacity * 64, "stats"},
                                                                        {pos, C * capacity * 16, "pos"},
                                                                        {result, 32, "result"},
                                                                        {workspace, need, "workspace"}};
  for (int i = 0; i < 5; i++) {
    HDF_CHECK_ARG(!hdf_overlap(out[i].p, out[i].n, ids, V * 4) && !hdf_overlap(out[i].p, out[i].n, image, C * V * 4),
                  "components: %s: %s overlaps an input", who, out[i].name);
    for (int j = i + 1; j < 5; j++)
      HDF_CHECK_ARG(!hdf_overlap(out[i].p, out[i].n, out[j].p, out[j].n), "components: %s: %s overlaps %s", who, out[i].name,
                    out[j].name);
  }
  return hdf_launch_cc_measure(ids, image, C, D, H, W, capacity, (long long*)geom, stats, (long long*)pos,
                               (unsigned long long*)result, workspace, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------- order statistics under an id map
// q is a host pointer: checked, and read, before anything is launched.
int64_t hdf_cc_quantiles_workspace_bytes(int C, int64_t capacity, int Q) {
  if (C < 1 || C > HDF_MEASURE_MAX_CHANNELS || capacity < 1 || capacity > HDF_MEASURE_MAX_CAPACITY || Q < 1 ||
      Q > HDF_QUANTILES_MAX_LEVELS) {
    hdf_set_error("components: quantiles: C = %d (1..%d), capacity %lld (1..%lld), Q = %d (1..%d)", C, HDF_MEASURE_MAX_CHANNELS,
                  (long long)capacity, (long long)HDF_MEASURE_MAX_CAPACITY, Q, HDF_QUANTILES_MAX_LEVELS);
    return -1;
  }
  return hdf_cc_quantiles_ws_bytes(capacity);
}
int hdf_cc_quantiles(const int32_t* ids, const float* image, int C, int D, int H, int W, int64_t capacity, const double* q, int Q,
                     int64_t* count, double* values, uint64_t* result, void* workspace, int64_t workspace_bytes,
                     hdf_stream stream) {
  const char* who = "quantiles";
  HDF_CHECK_ARG(C >= 1 && C <= HDF_MEASURE_MAX_CHANNELS, "components: %s: C = %d (1..%d)", who, C, HDF_MEASURE_MAX_CHANNELS);
  HDF_TRY(hdf_vol_check_dims(CC, who, D, H, W));
  HDF_CHECK_ARG(capacity >= 1 && capacity <= HDF_MEASURE_MAX_CAPACITY, "components: %s: capacity %lld (1..%lld)", who,
                (long long)capacity, (long long)HDF_MEASURE_MAX_CAPACITY);
  HDF_CHECK_ARG(Q >= 1 && Q <= HDF_QUANTILES_MAX_LEVELS, "components: %s: Q = %d (1..%d)", who, Q, HDF_QUANTILES_MAX_LEVELS);
  HDF_TRY(check_nonnull(CC, who, ids && image && q && count && values && result));
  for (int i = 0; i < Q; i++)   // (a NaN fails both comparisons)
    HDF_CHECK_ARG(q[i] >= 0.0 && q[i] <= 1.0, "components: %s: level %d is %g (0..1)", who, i, q[i]);
  const int64_t need = hdf_cc_quantiles_ws_bytes(capacity), V = (int64_t)D * H * W;
  HDF_TRY(check_workspace(CC, who, workspace, workspace_bytes, need));
  HDF_TRY(check_aligned8(CC, who, "count", count));
  HDF_TRY(check_aligned8(CC, who, "values", values));
  HDF_TRY(check_aligned8(CC, who, "result", result));
  const struct { const void* p; int64_t n; const char* name; } out[4] = {{count, capacity * 8, "count"},
                                                                        {values, C * capacity * Q * 24, "values"},
                                                                        {result, 32, "result"},
                                                                        {workspace, need, "workspace"}};
  for (int i = 0; i < 4; i++) {
    HDF_CHECK_ARG(!hdf_overlap(out[i].p, out[i].n, ids, V * 4) && !hdf_overlap(out[i].p, out[i].n, image, C * V * 4),
                  "components: %s: %s overlaps an input", who, out[i].name);
    for (int j = i + 1; j < 4; j++)
      HDF_CHECK_ARG(!hdf_overlap(out[i].p, out[i].n, out[j].p, out[j].n), "components: %s: %s overlaps %s", who, out[i].name,
                    out[j].name);
  }
  return hdf_launch_cc_quantiles(ids, image, C, D, H, W, capacity, q, Q, (long long*)count, values, (unsigned long long*)result,
                                 workspace, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------- per-lesion surface distances
// lesions is a host pointer: its rows are checked, and read, before anything else that depends on them.
int64_t hdf_lesion_surface_workspace_bytes(const int32_t* lesions, int64_t L, int D, int H, int W, int mm) {
  LesionPlan plan;
  const char* who = "lesion_workspace_bytes";
  if (hdf_vol_check_dims(SURF, who, D, H, W) != HDF_OK) return -1;
  if (L < 0 || (L > 0 && !lesions) || (mm != 0 && mm != 1)) {
    hdf_set_error("surface: %s: L = %lld, lesions %s, mm = %d (L >= 0, rows for L > 0, mm 0 or 1)", who, (long long)L,
                  lesions ? "given" : "null", mm);
    return -1;
  }
  return hdf_lesion_surface_plan(who, lesions, L, D, H, W, mm != 0, &plan) == HDF_OK ? plan.total : -1;
}
int hdf_lesion_surface(const int32_t* ids_pred, const int32_t* ids_truth, const uint8_t* truth_mask, int D, int H, int W,
                       const int64_t* pairs, int64_t n_pairs, const int32_t* lesions, int64_t L, const double* spacing,
                       void* workspace, int64_t workspace_bytes, uint64_t* results, hdf_stream stream) {
  const char* who = "lesion_surface";
  SurfaceSpacing sp;
  if (spacing) HDF_TRY(hdf_surface_check_spacing(who, spacing, &sp));
  HDF_TRY(hdf_vol_check_dims(SURF, who, D, H, W));
  HDF_CHECK_ARG(L >= 0 && n_pairs >= 0, "surface: %s: L = %lld, n_pairs = %lld (neither may be negative)", who, (long long)L,
                (long long)n_pairs);
  HDF_TRY(check_nonnull(SURF, who, ids_pred && ids_truth && truth_mask && (n_pairs == 0 || pairs) && (L == 0 || (lesions && results))));
  LesionPlan plan;
  HDF_TRY(hdf_lesion_surface_plan(who, lesions, L, D, H, W, spacing != nullptr, &plan));
  if (L == 0) return HDF_OK;   // nothing to carve, nothing to write
  HDF_TRY(check_workspace(SURF, who, workspace, workspace_bytes, plan.total));
  const int64_t V = (int64_t)D * H * W, rows = L * 12 * 8;
  HDF_TRY(check_disjoint(SURF, who, results, rows, workspace, plan.total, "results overlaps the workspace"));
  const struct { const void* p; int64_t n; } in[4] = {{ids_pred, V * 4}, {ids_truth, V * 4}, {truth_mask, V}, {pairs, n_pairs * 32}};
  for (int i = 0; i < 4; i++) {
    if (!in[i].p) continue;
    HDF_TRY(check_disjoint(SURF, who, results, rows, in[i].p, in[i].n, "results overlaps an input"));
    HDF_TRY(check_disjoint(SURF, who, workspace, plan.total, in[i].p, in[i].n, "workspace overlaps an input"));
  }
  return hdf_launch_lesion_surface(ids_pred, ids_truth, truth_mask, H, W, (const long long*)pairs, n_pairs, plan,
                                   spacing ? &sp : nullptr, workspace, (unsigned long long*)results, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------- binary morphology
int64_t hdf_morph_workspace_bytes(int D, int H, int W) {
  return ws_bytes_or_minus1(MORPH, "workspace_bytes", D, H, W, hdf_morph_ws_bytes);
}
int hdf_morph(const uint8_t* volume, int label, int op, int connectivity, int iterations, int border_value, int mode, int D,
              int H, int W, uint8_t* out, uint64_t* result, void* workspace, int64_t workspace_bytes, hdf_stream stream) {
  HDF_TRY(hdf_vol_check_dims(MORPH, "morph", D, H, W));
  HDF_CHECK_ARG(op == HDF_MORPH_DILATE || op == HDF_MORPH_ERODE || op == HDF_MORPH_OPEN || op == HDF_MORPH_CLOSE,
                "morphology: morph: op %d (HDF_MORPH_DILATE, _ERODE, _OPEN or _CLOSE)", op);
  HDF_TRY(hdf_morph_check_mask_args("morph", label, connectivity, mode));
  HDF_CHECK_ARG(iterations >= 1 && iterations <= HDF_MORPH_MAX_ITER, "morphology: morph: iterations %d (1..%d)", iterations,
                HDF_MORPH_MAX_ITER);
  HDF_CHECK_ARG(border_value == 0 || border_value == 1, "morphology: morph: border_value %d (0 or 1)", border_value);
  HDF_TRY(morph_check_buffers("morph", volume, out, result, workspace, workspace_bytes, hdf_morph_ws_bytes(D, H, W),
                              (int64_t)D * H * W));
  return hdf_launch_morph(volume, label, op, connectivity, iterations, border_value, mode, D, H, W, out,
                          (unsigned long long*)result, workspace, (hipStream_t)stream);
}
int64_t hdf_fill_holes_workspace_bytes(int D, int H, int W) {
  return ws_bytes_or_minus1(MORPH, "workspace_bytes", D, H, W, hdf_fill_holes_ws_bytes);
}
int hdf_fill_holes(const uint8_t* volume, int label, int connectivity, int mode, int D, int H, int W, uint8_t* out,
                   uint64_t* result, void* workspace, int64_t workspace_bytes, hdf_stream stream) {
  HDF_TRY(hdf_vol_check_dims(MORPH, "fill_holes", D, H, W));
  HDF_TRY(hdf_morph_check_mask_args("fill_holes", label, connectivity, mode));
  HDF_TRY(morph_check_buffers("fill_holes", volume, out, result, workspace, workspace_bytes, hdf_fill_holes_ws_bytes(D, H, W),
                              (int64_t)D * H * W));
  return hdf_launch_fill_holes(volume, label, connectivity, mode, D, H, W, out, (unsigned long long*)result, workspace,
                               (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------- lesion candidates
int64_t hdf_detect_workspace_bytes(int D, int H, int W) {
  return ws_bytes_or_minus1(DET, "workspace_bytes", D, H, W, hdf_detect_ws_bytes);
}
int hdf_detect_candidates(const float* prob, int D, int H, int W, int num_lesions, double factor, double stop, int connectivity,
                          int remove_adjacent, int64_t min_voxels, int first_round, int rounds, float* detection_map,
                          int32_t* indexed, int64_t* table, int64_t table_rows, uint64_t* result, void* workspace,
                          int64_t workspace_bytes, hdf_stream stream) {
  const char* who = "candidates";
  HDF_TRY(hdf_vol_check_dims(DET, who, D, H, W));
  HDF_CHECK_ARG(num_lesions >= 1, "detect: %s: num_lesions %d (at least 1)", who, num_lesions);
  HDF_CHECK_ARG(std::isfinite(factor) && factor > 1.0, "detect: %s: factor %g (finite, above 1)", who, factor);
  HDF_CHECK_ARG(std::isfinite(stop) && stop > 0.0, "detect: %s: stop %g (finite, above 0)", who, stop);
  HDF_CHECK_ARG(connectivity == 6 || connectivity == 18 || connectivity == 26, "detect: %s: connectivity %d (6, 18 or 26)", who,
                connectivity);
  HDF_CHECK_ARG(remove_adjacent == 0 || remove_adjacent == 1, "detect: %s: remove_adjacent %d (0 or 1)", who, remove_adjacent);
  HDF_CHECK_ARG(min_voxels >= 0, "detect: %s: min_voxels %lld is negative", who, (long long)min_voxels);
  HDF_CHECK_ARG(rounds >= 1 && first_round >= 0 && table_rows >= 0 && table_rows < ((int64_t)1 << 31),
                "detect: %s: rounds %d, first_round %d, table_rows %lld (rounds >= 1, first_round >= 0, table_rows in 0..2^31-1)",
                who, rounds, first_round, (long long)table_rows);
  HDF_TRY(check_nonnull(DET, who, prob && detection_map && indexed && result && (table_rows == 0 || table)));
  const int64_t need = hdf_detect_ws_bytes(D, H, W), V = (int64_t)D * H * W;
  HDF_TRY(check_workspace(DET, who, workspace, workspace_bytes, need));
  HDF_TRY(check_aligned8(DET, who, "table", table));
  HDF_TRY(check_aligned8(DET, who, "result", result));
  const struct { const void* p; int64_t n; const char* name; } buf[6] = {
      {prob, V * 4, "prob"},     {detection_map, V * 4, "detection_map"}, {indexed, V * 4, "indexed"},
      {table, table_rows * HDF_DETECT_TABLE_COLS * 8, "table"}, {result, 32, "result"}, {workspace, need, "workspace"}};
  for (int i = 0; i < 6; i++)
    for (int j = i + 1; j < 6; j++)
      HDF_CHECK_ARG(buf[i].n == 0 || buf[j].n == 0 || !hdf_overlap(buf[i].p, buf[i].n, buf[j].p, buf[j].n),
                    "detect: %s: %s overlaps %s", who, buf[i].name, buf[j].name);
  DetectArgs args;
  args.num_lesions = num_lesions, args.connectivity = connectivity, args.remove_adjacent = remove_adjacent;
  args.first_round = first_round, args.rounds = rounds, args.factor = factor, args.stop = stop;
  args.min_voxels = min_voxels, args.table_rows = table_rows;
  return hdf_launch_detect(prob, D, H, W, args, detection_map, indexed, (long long*)table, (unsigned long long*)result,
                           workspace, (hipStream_t)stream);
}

}  // extern "C"
