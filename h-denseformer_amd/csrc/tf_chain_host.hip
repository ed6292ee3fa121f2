// Host side of the persistent chain kernels (tf_chain.h): the fragment-major weight pack, the sizes and support predicates
// of transformer.h, and chain_launch -- the one place a persistent launch is issued from, so that the serialisation state
// below exists once per process, for both directions.
#include <mutex>

#include "tf_chain.h"

namespace {

// grid (layers + blocks, modalities, z), 256 threads: wave w of slice z copies the units u = 4 z + w (mod 4 gridDim.z) of its slot.
// Row fragment (wload): lane (i, g) <- W[n0 + i][g KQ + s0 + 4 j .. + 3]; column fragment (cload): element e of the lane's
// float4 <- W[g OQ + s0 + 4 j + e][n0 + i].
__global__ __launch_bounds__(256) void tf_chain_pack_kernel(ChainW cw, const float* __restrict__ params, int64_t mstride,
                                                            int DM, int nl, float4* __restrict__ wpack) {
  HDF_LIGHT_PRIO();   // (runs beside the first level-0 conv since round 5: exec.hip forward3d)
  const int m = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
  const int DMF = DM + 128, M = gridDim.y, nb = nl >> 2;
  auto rowf = [&](const float* W, int ldw, int n0, int KQ, int s0, int j) {
    return *reinterpret_cast<const float4*>(W + (int64_t)(n0 + i) * ldw + g * KQ + s0 + 4 * j);
  };
  auto colf = [&](const float* W, int ldw, int n0, int OQ, int s0, int j) {
    const float* q = W + (int64_t)(g * OQ + s0 + 4 * j) * ldw + n0 + i;
    return make_float4(q[0], q[ldw], q[2 * ldw], q[3 * ldw]);
  };
  if ((int)blockIdx.x < nl) {
    const int L = blockIdx.x, b = L >> 2, l = L & 3, Kq = DM + 32 * l;
    const float* w0 = chain_w0(cw, const_cast<float*>(params), b, l) + (int64_t)m * mstride;
    const float* rest = w0 + 32 * Kq;
    float4* dst = wpack + ((int64_t)m * nl + L) * (CH_SLOT * 64);
    for (int u = blockIdx.z * 4 + wave; u < CH_SLOT; u += 4 * gridDim.z) {
      float4 v;
      if (u < CH_W2) {
        v = rowf(rest + CO_WOUT, 32, 16 * ((u - CH_WO) >> 1), 8, 0, (u - CH_WO) & 1);
      } else if (u < CH_W1) {
        v = rowf(rest + CO_W2, 64, 16 * ((u - CH_W2) >> 2), 16, 0, (u - CH_W2) & 3);
      } else if (u < CH_WQ) {
        v = rowf(rest + CO_W1, 32, 16 * ((u - CH_W1) >> 1), 8, 0, (u - CH_W1) & 1);
      } else if (u < CH_W0) {
        v = rowf(rest + CO_WQKV, 32, 16 * ((u - CH_WQ) >> 1), 8, 0, (u - CH_WQ) & 1);
      } else if (u < CB_Q) {
        const int f = (u - CH_W0) / 11, j = (u - CH_W0) - f * 11;
        if (j >= (Kq >> 5)) continue;
        v = rowf(w0, Kq, 16 * (f & 1), Kq >> 2, (f >> 1) * (Kq >> 3), j);
      } else if (u < CB_W0) {
        const int f = (u - CB_Q) / 3, j = (u - CB_Q) - f * 3;
        v = colf(rest + CO_WQKV, 32, 16 * (f & 1), 24, 12 * (f >> 1), j);
      } else if (u < CB_W2) {
        const int t = (u - CB_W0) >> 1, j = (u - CB_W0) & 1;
        if (16 * t >= Kq) continue;
        v = colf(w0, Kq, 16 * t, 8, 0, j);
      } else if (u < CB_W1) {
        v = colf(rest + CO_W2, 64, 16 * ((u - CB_W2) >> 1), 8, 0, (u - CB_W2) & 1);
      } else if (u < CB_WO) {
        const int f = (u - CB_W1) >> 1;
        v = colf(rest + CO_W1, 32, 16 * (f & 1), 16, 8 * (f >> 1), (u - CB_W1) & 1);
      } else {
        const int f = u - CB_WO;
        v = colf(rest + CO_WOUT, 32, 16 * (f & 1), 8, 4 * (f >> 1), 0);
      }
      dst[u * 64 + lane] = v;
    }
  } else {
    const int b = blockIdx.x - nl;
    const TfOutP po = chain_out(cw, const_cast<float*>(params), b);
    const float* wa = po.wa + (int64_t)m * mstride;
    const float* wb = po.wb + (int64_t)m * mstride;
    float4* dst = wpack + (int64_t)M * nl * (CH_SLOT * 64) + ((int64_t)m * nb + b) * (CO_SLOT * 64);
    const int nja = DMF >> 4, ntb = DM >> 4;
    for (int u = blockIdx.z * 4 + wave; u < CO_SLOT; u += 4 * gridDim.z) {
      float4 v;
      if (u < OB_F) {
        const int t = u / 24, j = u - t * 24;
        if (j >= nja) continue;
        v = rowf(wa, DMF, 16 * t, DMF >> 2, 0, j);
      } else if (u < OB_B) {
        const int t = (u - OB_F) >> 2;
        if (t >= ntb) continue;
        v = rowf(wb, 64, 16 * t, 16, 0, (u - OB_F) & 3);
      } else if (u < OA_B) {
        const int t = (u - OB_B) >> 4, j = (u - OB_B) & 15;
        if (j >= ntb) continue;
        v = colf(wb, 64, 16 * t, DM >> 2, 0, j);
      } else {
        const int t = (u - OA_B) >> 2;
        if (t >= nja) continue;
        v = colf(wa, DMF, 16 * t, 16, 0, (u - OA_B) & 3);
      }
      dst[u * 64 + lane] = v;
    }
  }
}

}  // namespace

size_t tf_chain_sync_bytes(const TfDims& d) { return (size_t)(d.M * d.B + 1) * SYNC_LINE * sizeof(unsigned); }
size_t tf_chain_frag_bytes(const TfDims& d, int nb) {
  const size_t nt = ceil_div(d.N, TT);
  return (size_t)nb * 4 * d.M * d.B * (nt * 8 * FR_W + 8 * nt * TT) * sizeof(float);   // records + the -lse rows
}
bool tf_chain_backward_supported(const TfDims& d, int dtype) {
  // (16-bit modes: the hand-off records must fit tf_scratch = rows x 160 floats; whole tiles always do)
  return tf_chain_supported(d) && chain_bwd_lds(d, dtype) <= LDS_LIMIT &&
         (dtype == HDF_F32 || ((size_t)2 * d.M * d.B * ceil_div(d.N, TT) * (8 * XG_W + 8 * TT) <= (size_t)d.M * d.B * d.N * 160 &&
                               attn_rows(d.N) <= 1024));
}
size_t tf_chain_wpack_bytes(const TfDims& d, int nb) {
  return ((size_t)d.M * nb * 4 * CH_SLOT + (size_t)d.M * nb * CO_SLOT) * 64 * sizeof(float4);
}

// what the kernels can address, whatever the grid
bool tf_chain_shape_ok(const TfDims& d) {
  return d.DM % 32 == 0 && d.DM >= 32 && d.DM <= 256 && d.N >= 1 && (int64_t)d.N * 96 * 4 < ((int64_t)1 << 31);
}
// ... and every workgroup of the grid resident at once: one compute unit each (512 threads at ~250 registers fill a unit's
// register files), so tiles <= the units the launch may assume -- hdf_cu_budget(), capped by the device's own count
bool tf_chain_supported(const TfDims& d) {
  return tf_chain_shape_ok(d) && d.M * d.B * ceil_div(d.N, TT) <= hdf_cu_budget();
}

int tf_chain_pack(const TfDims& d, const TfChainP& cp, int nb, const float* params, void* wpack, hipStream_t st) {
  ChainW w{};
  HDF_CHECK_ARG(chain_digest(cp, d.DM, w), "transformer chain: irregular parameter layout");
  hipLaunchKernelGGL(tf_chain_pack_kernel, dim3(nb * 4 + nb, d.M, 8), dim3(256), 0, st, w, params, d.mstride, d.DM, nb * 4,
                     reinterpret_cast<float4*>(wpack));
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

// At most ONE persistent transformer launch in flight per device and process: two of them resident together
// -- two plans or models on different streams -- can each hold a part of the compute units and wait for siblings that are
// never dispatched.  Every launch therefore waits for the event of the previous persistent launch of the process on the
// same device and records its own, under a mutex (launches of one stream are ordered anyway: the wait is then free).
// Another PROCESS on the same device is outside this chain: that case ends in the give-up path of chain_wait.
namespace {
struct ChainSerial {
  std::mutex mu;
  hipEvent_t last[16] = {};
  bool armed[16] = {};
};
ChainSerial g_chain_serial;
// orders `st` behind the previous persistent launch; chain_serial_done right after the launch (both under the lock)
int chain_serial_enter(hipStream_t st, int& dev) {
  dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = 0;
  if (g_chain_serial.armed[dev] && hipStreamWaitEvent(st, g_chain_serial.last[dev], 0) != hipSuccess) {
    hdf_set_error("transformer chain: could not order the launch behind the previous persistent launch");
    return HDF_ERR_HIP;
  }
  return HDF_OK;
}
int chain_serial_done(hipStream_t st, int dev) {
  if (!g_chain_serial.last[dev] &&
      hipEventCreateWithFlags(&g_chain_serial.last[dev], hipEventDisableTiming) != hipSuccess) {
    g_chain_serial.last[dev] = nullptr;
    hdf_set_error("transformer chain: could not create the serialisation event");
    return HDF_ERR_HIP;
  }
  if (hipEventRecord(g_chain_serial.last[dev], st) != hipSuccess) {
    hdf_set_error("transformer chain: could not record the serialisation event");
    return HDF_ERR_HIP;
  }
  g_chain_serial.armed[dev] = true;
  return HDF_OK;
}
}  // namespace

int chain_launch(const void* kern, void* args, int grid, size_t shm, const TfDims& d, unsigned* sync, hipStream_t st) {
  HDF_TRY(allow_lds(kern, shm));
  std::lock_guard<std::mutex> lock(g_chain_serial.mu);
  int dev = 0;
  HDF_TRY(chain_serial_enter(st, dev));
  hipError_t e = hipMemsetAsync(sync, 0, tf_chain_sync_bytes(d), st);
  if (e != hipSuccess) {
    hdf_set_error("transformer chain: hipMemsetAsync failed: %s", hipGetErrorString(e));
    return HDF_ERR_HIP;
  }
  void* kargs[] = {args};
  (void)hipLaunchKernel(kern, dim3(grid), dim3(CT), kargs, shm, st);   // (its status: HDF_LAUNCH_CHECK)
  HDF_LAUNCH_CHECK();
  return chain_serial_done(st, dev);
}
