// EXPERIMENT, not part of the product: the in-place LoRA up-projection  Y[T, N] += scale_seg * XA[T, r-range] . M[n, :]^T
// per column segment as one MFMA kernel (one read + one write of Y), written as the third kernel beside dta_lora_down / dta_lora_wgrad.
// scripts/lora_probe.py measured it at 0.25-0.56x of torch's addmm_ (hipBLASLt) at every bench shape, so the product ships addmm_.  Kept
// so that the measurement can be repeated:
//   hipcc --offload-arch=gfx950 -O3 -fPIC -shared -std=c++17 -o scripts/diag/liblora_up_add_experiment.so scripts/diag/lora_up_add_experiment.hip
// and scripts/lora_probe.py picks the library up when it is there.  Why it loses: the accumulator layout of the 32x32 MFMA leaves a lane
// 2-byte accesses to Y (64 contiguous bytes per row and instruction), and with K = r there is no arithmetic to hide them behind.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
constexpr int MAXR = 256, MAXSEG = 8, BM = 128, BK = 64, KF_LD = BK + 8;

__device__ __forceinline__ uint4 ld8(const uint16_t* base, int64_t row, int64_t ld, int c, int clim, bool vec) {
  uint4 r = {0, 0, 0, 0};
  if (c >= clim) return r;
  const uint16_t* p = base + row * ld + c;
  if (vec && c + 8 <= clim) return *reinterpret_cast<const uint4*>(p);
  uint32_t e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = c + j < clim ? (uint32_t)p[j] : 0u;
  r.x = e[0] | (e[1] << 16); r.y = e[2] | (e[3] << 16); r.z = e[4] | (e[5] << 16); r.w = e[6] | (e[7] << 16);
  return r;
}
__device__ __forceinline__ bf16x8 frag_kfast(const char* img, int ob, int s, int lane) {
  return *reinterpret_cast<const bf16x8*>(img + ((ob * 32 + (lane & 31)) * KF_LD + 16 * s + 8 * (lane >> 5)) * 2);
}

struct UpArgs {
  void* y; const uint16_t *xa, *m;
  int64_t ldy, ldxa, ldm;
  int T, vxa, vm, nseg;
  int n0[MAXSEG], nlen[MAXSEG], r0[MAXSEG], rlen[MAXSEG], tile0[MAXSEG];
  float scale[MAXSEG];
};

// 128 x 128 tiles (4 waves of 64 x 64); the grid's y axis counts the tiles of the segments one after another
__global__ __launch_bounds__(256) void up_add_k(UpArgs a) {
  __shared__ __attribute__((aligned(16))) char lds_a[BM * KF_LD * 2];
  __shared__ __attribute__((aligned(16))) char lds_b[BM * KF_LD * 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  int seg = 0;
  for (int s = 1; s < a.nseg; ++s) if ((int)blockIdx.y >= a.tile0[s]) seg = s;
  const int m0 = blockIdx.x * BM;
  const int n0 = a.n0[seg] + ((int)blockIdx.y - a.tile0[seg]) * BM, nlim = a.n0[seg] + a.nlen[seg];
  const int r0 = a.r0[seg], klim = a.rlen[seg];
  const float scale = a.scale[seg];
  const bool vxa = a.vxa && (r0 & 7) == 0;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  uint4 sa[4], sb[4];
  auto load = [&](int kb) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int v = tid + 256 * i, o = v >> 3, kc = (v & 7) * 8;
      sa[i] = m0 + o < a.T ? ld8(a.xa + r0, m0 + o, a.ldxa, kb + kc, klim, vxa) : uint4{0, 0, 0, 0};
      sb[i] = n0 + o < nlim ? ld8(a.m, n0 + o, a.ldm, kb + kc, klim, a.vm) : uint4{0, 0, 0, 0};
    }
  };
  load(0);
  for (int kb = 0; kb < klim; kb += BK) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int v = tid + 256 * i, off = ((v >> 3) * KF_LD + (v & 7) * 8) * 2;
      *reinterpret_cast<uint4*>(lds_a + off) = sa[i]; *reinterpret_cast<uint4*>(lds_b + off) = sb[i];
    }
    __syncthreads();
    if (kb + BK < klim) load(kb + BK);
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      if (kb + 16 * s >= klim) break;
      bf16x8 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) { fa[i] = frag_kfast(lds_a, 2 * wm + i, s, lane); fb[i] = frag_kfast(lds_b, 2 * wn + i, s, lane); }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
  }
  __bf16* Y = reinterpret_cast<__bf16*>(a.y);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 64 + j * 32 + (lane & 31);
      if (n >= nlim) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 64 + i * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
        if (m < a.T) { __bf16* p = Y + (int64_t)m * a.ldy + n; *p = (__bf16)((float)*p + scale * acc[i][j][r]); }
      }
    }
}
inline int vec_ok(const void* p, int64_t ld) { return ((uintptr_t)p & 15) == 0 && ld % 8 == 0; }
}  // namespace

// bf16 only.  seg_host: nseg x {n0, nlen, r0, rlen} (ascending, disjoint, multiples of 16 in n); returns 0, -1 (arguments), -2 (shape), -4 (launch)
extern "C" int lora_up_add_experiment(void* y, int64_t ldy, const void* xa, int64_t ldxa, const void* m, int64_t ldm, int32_t nseg,
                                      const int32_t* seg_host, const float* seg_scale_host, int32_t T, int32_t N, void* stream) {
  if (T <= 0 || N <= 0 || nseg <= 0 || !y || !xa || !m || !seg_host || !seg_scale_host || ldy < N) return -1;
  if (nseg > MAXSEG || N % 16) return -2;
  UpArgs a{};
  a.y = y; a.xa = (const uint16_t*)xa; a.m = (const uint16_t*)m; a.ldy = ldy; a.ldxa = ldxa; a.ldm = ldm;
  a.T = T; a.vxa = vec_ok(xa, ldxa); a.vm = vec_ok(m, ldm); a.nseg = nseg;
  int tiles = 0, prev_end = 0;
  for (int s = 0; s < nseg; ++s) {
    const int n0 = seg_host[4 * s], nlen = seg_host[4 * s + 1], r0 = seg_host[4 * s + 2], rlen = seg_host[4 * s + 3];
    if (n0 < prev_end || nlen <= 0 || n0 + nlen > N || r0 < 0 || rlen <= 0 || r0 + rlen > ldxa || rlen > ldm) return -1;
    if (rlen > MAXR || n0 % 16 || nlen % 16) return -2;
    a.n0[s] = n0; a.nlen[s] = nlen; a.r0[s] = r0; a.rlen[s] = rlen; a.tile0[s] = tiles; a.scale[s] = seg_scale_host[s];
    tiles += (nlen + BM - 1) / BM; prev_end = n0 + nlen;
  }
  up_add_k<<<dim3((T + BM - 1) / BM, tiles), dim3(256), 0, (hipStream_t)stream>>>(a);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}
