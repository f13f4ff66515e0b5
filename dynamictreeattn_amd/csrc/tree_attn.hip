// Tree attention forward / backward for gfx950 (MI355X, CDNA4).  head_dim 128 or 64 (templated; see img_off_d), bf16 or f16.
//
// One kernel family serves both forms of the reference's "node attends to its ancestor path":
//   * packed trie (DFS pre-order): key s visible to query t  <=>  s <= t < subtree_end[s]
//   * stack form (tree_training_engine.py:171-186): subtree_end == NULL, q_offset = start
//
// Tiling (wave64, v_mfma_f32_32x32x16, two waves per SIMD everywhere):
//   fwd / dQ : workgroup = 8 waves = 128 query rows x the TWO query heads of one kv group (4 waves = 128 rows of one
//              head when the group is odd); each wave owns 32 rows with the QUERY ON THE MFMA LANE (S^T = K.Q^T), so
//              the softmax row statistics are lane-local and the S^T accumulator is directly the B operand of
//              O^T += V^T.P^T / dQ^T += K^T.dS^T.  Both heads share the staged 64-key K/V tiles.
//   dK/dV    : workgroup = 8 waves = 128 keys of one kv head with the KEY ON THE LANE (S = Q.K^T): the two 4-wave groups
//              own the same keys and split every 64-row query tile; dK^T/dV^T live in 128 accumulator registers per wave
//              across the whole query sweep (all query heads of the GQA group); the K/V fragments sit in LDS in fragment
//              order.  Heavy key tiles are cut into split-Q work units whose fp32 slabs a finalize launch sums in order:
//              no atomics, bitwise reproducible.
//   Tiles (K/V for fwd, Q/dO for dK/dV) go global -> LDS by LDS-DMA issued from INLINE ASM (dma_* below) into one
//   XOR-swizzled 256-B-row (D = 64: 128-B-row) image that serves BOTH row reads (ds_read_b128) and transposed reads (ds_read_b64_tr_b16);
//   the dQ kernel stages through registers (issue early, write late).
//
// Why inline asm for the DMA: with the builtin, hipcc (ROCm 7.2) waits `vmcnt(0)` for the in-flight prefetch of the
// NEXT tile in front of LDS reads of the CURRENT one (before the first ds_read when the kernel has a second __shared__
// object, before the first transposed / float4 read otherwise) - the prefetch was exposed on every tile.  An asm DMA is
// outside hipcc's bookkeeping (cdna guide 5.7): the only wait is our own `s_waitcnt vmcnt(0)` in front of the
// tile-end barrier, so a tile's DMA has the whole compute phase of the previous tile to land.
//
// Lane maps used here were verified on hardware by tests/micro/mfma_layout_probe.hip.
// The round-1 ablation switches (-DDTA_ABL) and the retired 4-wave dK/dV kernel were frozen copies of this file (last
// present in 4de734c); the A/B forward forms 3 and 4 were removed (last present in b0d42b7).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "dta_common.h"
#include "dta_device.h"

// Diagnostic build switch (-DDTA_STAMP=1): in-kernel s_memtime stamps at the segment boundaries of the forward's tile loop, summed per
// wave in scalar registers and written to a debug buffer of their own (cdna_hip_programming.md §7 "In-kernel stamps"); scripts/fwd_stamps.py
// reads the SHARES.  No stamp executes in the product build.
#if defined(DTA_STAMP) && DTA_STAMP
__device__ unsigned long long* dta_stamp_buf = nullptr;
extern "C" int dta_debug_set_stamp_buffer(void* p) { return hipMemcpyToSymbol(HIP_SYMBOL(dta_stamp_buf), &p, sizeof(p)) == hipSuccess ? 0 : -4; }
#define DTA_STAMP_DECL unsigned long long st_prev_, st_sum_[6] = {0, 0, 0, 0, 0, 0}; unsigned long long st_tiles_ = 0; \
  __builtin_amdgcn_sched_barrier(0); asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_prev_) :: "memory"); __builtin_amdgcn_sched_barrier(0);
#define DTA_STAMP_AT(K) { unsigned long long t_; __builtin_amdgcn_sched_barrier(0); asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); \
  __builtin_amdgcn_sched_barrier(0); st_sum_[K] += t_ - st_prev_; st_prev_ = t_; }
#define DTA_STAMP_TILE ++st_tiles_;
#define DTA_STAMP_STORE if (dta_stamp_buf && lane == 0) { unsigned long long* o_ = dta_stamp_buf + ((size_t)blockIdx.x * 8 + wave) * 8; \
  for (int k_ = 0; k_ < 6; ++k_) o_[k_] = st_sum_[k_]; o_[6] = st_tiles_; o_[7] = (unsigned long long)__builtin_amdgcn_s_getreg(0xF804) /* HW_ID: wave / simd / cu ids */; }
#else
#define DTA_STAMP_DECL
#define DTA_STAMP_AT(K)
#define DTA_STAMP_TILE
#define DTA_STAMP_STORE
#endif

namespace {

struct AttnParams {
  const void *q, *k, *v, *o, *dout;
  void *out, *dq, *dk, *dv;
  float *lse_w; const float* lse_r; float* delta;
  const int32_t *subtree_end, *run_ptr, *runs, *ktile_qend;
  const int32_t *dkv_units, *dkv_splits; float* dkv_ws;     // split-Q work units of the dK/dV sweep (NULL: one unit per key tile)
  int32_t Tq, Tk, q_offset, Hq, Hkv, group;
  int32_t hgroups, head0;          // forward / dQ launch: workgroups per (query tile, kv head) and the first query head (inside a kv group) they cover
  int64_t q_st, q_sh, kv_st, kv_sh, v_st, v_sh, o_st, o_sh, dq_st, dq_sh, dkv_st, dkv_sh;
  float scale; int32_t accumulate; int32_t ktile;
};
// Sliding-window form (window > 0): key s must also be >= the query row's lower bound, win_lo[row] (packed form)
// or q_offset + row - window + 1 (stack form, win_lo == NULL).  A parameter type of its own: the kernels without a window (WIN = false)
// keep the parent's kernel arguments, and every WIN term below folds away at compile time, so their device code is unchanged.
struct AttnParamsW : AttnParams { const int32_t* win_lo; int32_t window; };
// Soft-capped form (softcap > 0): the score is softcap * tanh(scale q.k / softcap), capped BEFORE the visibility
// mask.  Again parameter types of their own (with and without a window), so that the CAP = false kernels keep their arguments and code.
struct AttnParamsC : AttnParams { float softcap; };
struct AttnParamsWC : AttnParamsW { float softcap; };
template <bool WIN, bool CAP = false> using AttnP = typename std::conditional<CAP, typename std::conditional<WIN, AttnParamsWC, AttnParamsC>::type,
                                                                              typename std::conditional<WIN, AttnParamsW, AttnParams>::type>::type;

// Byte offset of 16-B chunk `ch` of row `row` in a [rows][D x 16-bit] image.  head_dim 128: 256-B rows (16 chunks); the XOR makes both the
// 32x32x16 row reads (ds_read_b128) and the transposed reads conflict-free.
// head_dim 64: the same image with 128-B rows (8 chunks).
// 16-B slot of chunk `pc` of row `row` in the 64 banks (256 B): 8 * (row & 1) + pc.  With pc = ch ^ f(row), f a 3-bit function of the row:
//   ds_read_b128 row reads (lane = row r of a 32-row block, all lanes of a group read the same logical chunk): the four lane groups are the
//     rows {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} (x2 for the lane halves); in each, the 8 rows of one parity have 8 distinct
//     r >> 1 (mod 8), so f must be a bijection of bits 1..3 of the row -> 16 distinct slots.
//   ds_read_b64_tr_b16 transposed reads (2 groups x 32 lanes): a group reads rows 4j..4j+3 x the four chunks 4mb..4mb+3; rows 4j and 4j+2
//     (and 4j+1, 4j+3) have the same parity and XOR the same aligned chunk quad onto itself unless bit 2 of f differs between them, i.e. bit 2
//     of f must follow row bit 1 -> 16 distinct slots.
//   f(row) = {row bit 1, row bit 3, row bit 2} (bits 2, 1, 0) meets both; it depends on row bits 1..3 only, so row offsets of 16 rows keep
//   every lane's swizzle (the FragOffsT property below).  The swizzle of the D = 128 image (16 chunks, 4-bit f of row bits 0..3) is unchanged.
__device__ __forceinline__ int swz64(int row) { return ((row & 2) << 1) | ((row >> 2) & 3); }
template <int D> __device__ __forceinline__ int img_off_d(int row, int ch) {
  if constexpr (D == 128) return row * 256 + ((ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4);
  else { static_assert(D == 64, "head_dim 64 or 128"); return row * 128 + ((ch ^ swz64(row)) << 4); }
}
template <int D> constexpr int tile_bytes() { return 64 * 2 * D; }   // 64 rows x D x 2 B

template <class V8, int D> __device__ __forceinline__ V8 row_frag(const char* img, int row, int ch) {
  return *reinterpret_cast<const V8*>(img + img_off_d<D>(row, ch));
}

// A-operand fragment read TRANSPOSED from the image: A[m = 32*mb + (lane&31)][kk], where the 16-deep
// k-step covers image rows R0..R0+15 in the accumulator-as-operand order
// (element j of lane half h <-> image row R0 + 8*(j>>2) + 4*h + (j&3)) and m indexes image columns.
template <class V8, int D> __device__ __forceinline__ V8 tr_frag(const char* img, int R0, int mb, int lane) {
  const int G = lane >> 4, hh = lane >> 5, i = lane & 15, qd = i >> 2, p = i & 3;
  const int ch = 4 * mb + 2 * (G & 1) + (p >> 1);
  const int ra = R0 + 4 * hh + qd;
  s16x4 lo = tr_read(img + img_off_d<D>(ra, ch) + 8 * (p & 1));
  s16x4 hi = tr_read(img + img_off_d<D>(ra + 8, ch) + 8 * (p & 1));
  s16x8 both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(V8, both);
}

// accumulator registers 8*s2 .. 8*s2+7 -> 16-bit fragment of k-step s2 (s2 = 0,1) of a 32-row block
template <int DT> __device__ __forceinline__ typename Ty<DT>::v8 pack_half(const f32x16& x, int s2) {
  typename Ty<DT>::v8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (typename Ty<DT>::e)x[8 * s2 + j];
  return r;
}

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// The cap's two constants: kcap turns a raw q.k into tanh's argument a (2 log2(e) scale / softcap), and the log2-domain score factor c
// becomes softcap log2(e).  Without a cap the one statement the kernels had (c = scale log2(e)) is all that is left.
#define DTA_CAP_CONSTANTS                                                                                  \
  const float c = (CAP ? cap_of(p) : p.scale) * LOG2E;                                                     \
  [[maybe_unused]] const float kcap = CAP ? 2.f * LOG2E * p.scale / cap_of(p) : 0.f;
template <class P> __device__ __forceinline__ float cap_of(const P& p) {
  if constexpr (std::is_base_of<AttnParamsC, P>::value || std::is_base_of<AttnParamsWC, P>::value) return p.softcap; else return 0.f;
}

// ---- iterator over the 64-key tiles of a query tile's run list --------------------------------
struct TileIter {
  const int32_t* runs; int ri, re;      // run cursor
  int k0, kend, flag;                   // current tile
  int diag_first_q;                     // NULL-run mode: packed index of the tile's first query (-64 with a subtree bound:
                                        // then every tile needs the mask, below the diagonal too)
  __device__ __forceinline__ bool load_run() {
    while (ri < re) {
      k0 = __builtin_amdgcn_readfirstlane(runs[4 * ri]); kend = __builtin_amdgcn_readfirstlane(runs[4 * ri + 1]);
      flag = __builtin_amdgcn_readfirstlane(runs[4 * ri + 2]);       // workgroup-uniform: keep the cursor in SGPRs
      if (k0 < kend) return true;
      ++ri;
    }
    return false;
  }
  __device__ __forceinline__ bool advance() {          // to the next tile; false when exhausted
    k0 += 64;
    if (k0 < kend) return true;
    if (runs == nullptr) return false;
    ++ri;
    return load_run();
  }
  __device__ __forceinline__ bool masked() const {
    if (runs == nullptr) return (k0 + 63 > diag_first_q) || (k0 + 64 > kend);
    return flag != 0 || (k0 + 64 > kend);
  }
};

// Deferred reference maximum of the forward (log2 domain): the running reference follows a tile's row maximum only when that exceeds it by
// more than this, so P <= 2^THR (fp32 sums; bf16 P keeps its relative precision) and the rescale of O - taken on nine tiles in ten with
// THR = 0, because ANY of a wave's rows triggers it - becomes rare.  -DDTA_FWD_THR=0 restores the exact-maximum form.
#ifndef DTA_FWD_THR
#define DTA_FWD_THR 4.0f
#endif
constexpr float FWD_THR = DTA_FWD_THR;
constexpr int SE_BYTES = 256;                                       // 64 x int32 subtree_end of the staged keys

__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
__device__ __forceinline__ float half_max(float x) {      // max(x, value of the lane 32 away) by v_permlane32_swap (no LDS round trip)
  const unsigned u = __float_as_uint(x);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

// Per-lane byte offsets of every fragment read inside one image, computed once: the XOR swizzle depends on the
// lane only (row blocks of 32 and k-steps of 16 rows leave row&3 and (row>>2)&3 unchanged), so inside the tile
// loop every ds_read is <lane offset register> + <compile-time immediate>.  row[s]: k-step s (D/16 of them) of a row read;
// tr[mb], tr[D/32 + mb]: low / high half of the transposed read of 32-column block mb.
template <int D> struct FragOffsT { int row[D / 16]; int tr[D / 16]; };
template <int D> __device__ __forceinline__ FragOffsT<D> frag_offsets(int lane) {
  FragOffsT<D> o;
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int s = 0; s < D / 16; ++s) o.row[s] = img_off_d<D>(r, 2 * s + h);
  const int G = lane >> 4, i = lane & 15, qd = i >> 2, pp = i & 3;
#pragma unroll
  for (int mb = 0; mb < D / 32; ++mb) {
    const int ch = 4 * mb + 2 * (G & 1) + (pp >> 1);
    o.tr[mb] = img_off_d<D>(4 * h + qd, ch) + 8 * (pp & 1);
    o.tr[D / 32 + mb] = img_off_d<D>(4 * h + qd + 8, ch) + 8 * (pp & 1);
  }
  return o;
}
template <class V8> __device__ __forceinline__ V8 tr_pair(const char* lo_p, const char* hi_p) {
  s16x4 lo = tr_read(lo_p);
  s16x4 hi = tr_read(hi_p);
  s16x8 both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(V8, both);
}
template <class V8, int D> __device__ __forceinline__ V8 tr_frag_o(const char* img_r0, const FragOffsT<D>& o, int mb) {
  s16x4 lo = tr_read(img_r0 + o.tr[mb]);
  s16x4 hi = tr_read(img_r0 + o.tr[D / 32 + mb]);
  s16x8 both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(V8, both);
}

// ---- LDS-DMA from inline asm (see the file header for why) ---------------------------------------------------------
// A wave instruction lands 64 x 16 B = 1 KiB = 4 image rows lane-linearly at M0, so the image's XOR swizzle goes on the
// per-lane SOURCE chunk.  The global address is <scalar base> + <32-bit per-lane byte offset>: per tile only the base
// moves.  `s_nop 4` covers a base that was just produced by v_readfirstlane (VALU-written SGPR -> VMEM, 5 wait states),
// `s_nop 0` the M0 write -> LDS-DMA hazard.  hipcc does not count these loads: DMA_WAIT() before the barrier that
// publishes the tile is the only thing that orders them.
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char*)(p);
}
// pieces {0, 1} of image A (at lds, lds + 1 KiB) and of image B (at lds + tile_bytes<128>() = 16 KiB, + 1 KiB): the head_dim 128 tiles
__device__ __forceinline__ void dma_pair2(uint32_t oa0, uint32_t oa1, const void* ba, uint32_t ob0, uint32_t ob1, const void* bb, uint32_t lds) {
  asm volatile(
      "s_nop 4\n\t"
      "s_mov_b32 m0, %6\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %0, %4\n\t"
      "s_add_u32 m0, %6, 0x4000\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %2, %5\n\t"
      "s_add_u32 m0, %6, 0x400\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %4\n\t"
      "s_add_u32 m0, %6, 0x4400\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %3, %5"
      :: "v"(oa0), "v"(oa1), "v"(ob0), "v"(ob1), "s"(ba), "s"(bb), "s"(lds) : "memory", "scc");
}
// 64 dwords (row constants of a tile: subtree_end, lse, delta)
__device__ __forceinline__ void dma_dword(uint32_t off, const void* base, uint32_t lds) {
  asm volatile("s_nop 4\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" :: "v"(off), "s"(base), "s"(lds) : "memory");
}
#define DMA_WAIT() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

// Byte offset of this lane's 16-B chunk of image row `row` (rows of `stride` elements of `esz` bytes), swizzled as image row `img_row`.
// head_dim D: a 1-KiB piece is 1024 / (2 D) image rows of D / 8 chunks (D = 128: 4 rows, lane -> row lane >> 4, chunk lane & 15;
// D = 64: 8 rows, lane -> row lane >> 3, chunk lane & 7)
template <int D> __device__ __forceinline__ uint32_t dma_src_off_d(int row, int img_row, int lane, int64_t stride, int esz) {
  if constexpr (D == 128) return (uint32_t)((row * stride + ((lane & 15) ^ (((img_row & 3) << 2) | ((img_row >> 2) & 3))) * 8) * (int64_t)esz);
  else return (uint32_t)((row * stride + ((lane & 7) ^ swz64(img_row)) * 8) * (int64_t)esz);
}
template <int D> constexpr int dma_lane_row_shift() { return D == 128 ? 4 : 3; }
// one piece of image A (at lds) and one of image B (at lds + TB): the D = 64 tiles, whose waves own one piece per image (or an odd count)
template <int TB> __device__ __forceinline__ void dma_one2(uint32_t oa, const void* ba, uint32_t ob, const void* bb, uint32_t lds) {
  asm volatile(
      "s_nop 4\n\t"
      "s_mov_b32 m0, %4\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %0, %2\n\t"
      "s_add_u32 m0, %4, %5\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %3"
      :: "v"(oa), "v"(ob), "s"(ba), "s"(bb), "s"(lds), "n"(TB) : "memory", "scc");
}

// K/V tile pair of the forward: NW waves move the DH/8 + DH/8 pieces (DH = the kernel's head_dim: 16 + 16 at 128, 8 + 8 at 64); wave w owns
// pieces (DH/8/NW)*w .. of both images.
// subtree_end of the 64 keys goes by 4-byte DMA from wave 0; keys at or beyond the run end are excluded by the
// caller's `k <= min(q, kend-1)` test, not by a sentinel.
#define DTA_KV_PPW(NW) (DH / 8 / (NW))
#define DTA_KV_ROW(NW, I) ((512 / DH) * (wave * DTA_KV_PPW(NW) + (I)) + (lane >> dma_lane_row_shift<DH>()))
#define DTA_KV_OFFSETS(NW)                                                                                 \
  uint32_t voff_k[DTA_KV_PPW(NW)], voff_v[DTA_KV_PPW(NW)];                                                 \
  _Pragma("unroll") for (int i_ = 0; i_ < DTA_KV_PPW(NW); ++i_) {                                          \
    const int row_ = DTA_KV_ROW(NW, i_);                                                                   \
    voff_k[i_] = dma_src_off_d<DH>(row_, row_, lane, p.kv_st, sizeof(e));                                  \
    voff_v[i_] = dma_src_off_d<DH>(row_, row_, lane, p.v_st, sizeof(e)); }
#define DTA_KV_DMA(BASE, K0, NW)                                                                           \
  { char* base_ = (BASE); const int k0_ = (K0);                                                            \
    if (wave == 0) {                                                                                       \
      if (p.subtree_end) { int ki_ = k0_ + lane; ki_ = ki_ < p.Tk ? ki_ : p.Tk - 1;                        \
        dma_dword((uint32_t)ki_ * 4u, p.subtree_end, lds_addr(base_ + 2 * tile_bytes<DH>())); }           \
      else reinterpret_cast<int*>(base_ + 2 * tile_bytes<DH>())[lane] = 0x7fffffff; }                     \
    const char* kb_ = reinterpret_cast<const char*>(kbase) + (int64_t)k0_ * p.kv_st * (int64_t)sizeof(e);  \
    const char* vb_ = reinterpret_cast<const char*>(vbase) + (int64_t)k0_ * p.v_st * (int64_t)sizeof(e);   \
    uint32_t ok_[DTA_KV_PPW(NW)], ov_[DTA_KV_PPW(NW)];                                                     \
    _Pragma("unroll") for (int i_ = 0; i_ < DTA_KV_PPW(NW); ++i_) { ok_[i_] = voff_k[i_]; ov_[i_] = voff_v[i_]; } \
    if (k0_ + 64 > p.Tk) {                         /* ragged last tile of the tensor: clamp the row per lane */ \
      _Pragma("unroll") for (int i_ = 0; i_ < DTA_KV_PPW(NW); ++i_) {                                      \
        const int row_ = DTA_KV_ROW(NW, i_);                                                               \
        const int rr_ = k0_ + row_ < p.Tk ? row_ : p.Tk - 1 - k0_;                                         \
        ok_[i_] = dma_src_off_d<DH>(rr_, row_, lane, p.kv_st, sizeof(e)); ov_[i_] = dma_src_off_d<DH>(rr_, row_, lane, p.v_st, sizeof(e)); } } \
    if constexpr (DH == 128) {                                                                             \
      _Pragma("unroll") for (int i_ = 0; i_ < DTA_KV_PPW(NW); i_ += 2)                                     \
        dma_pair2(ok_[i_], ok_[i_ + 1], kb_, ov_[i_], ov_[i_ + 1], vb_, lds_addr(base_ + (wave * DTA_KV_PPW(NW) + i_) * 1024)); \
    } else {                                                                                               \
      _Pragma("unroll") for (int i_ = 0; i_ < DTA_KV_PPW(NW); ++i_)                                        \
        dma_one2<tile_bytes<DH>()>(ok_[i_], kb_, ov_[i_], vb_, lds_addr(base_ + (wave * DTA_KV_PPW(NW) + i_) * 1024)); } }

// The first DTA_V_PRELOAD_N V fragments (k-step by k-step) requested BEFORE the row maximum (they do not depend on the softmax; hipcc otherwise issues them right in
// front of the first PV MFMA, which then waits an LDS latency).  -DDTA_V_PRELOAD_N=0 disables.
#ifndef DTA_V_PRELOAD_N
#define DTA_V_PRELOAD_N 4
#endif
#if DTA_V_PRELOAD_N
#define DTA_V_PRELOAD v8 vpre_[DTA_V_PRELOAD_N]; _Pragma("unroll") for (int i_ = 0; i_ < DTA_V_PRELOAD_N; ++i_) { vpre_[i_] = tr_frag_o<v8>(Vs + 32 * DH * (i_ / (DH / 32)), offs, i_ % (DH / 32)); asm volatile("" : "+v"(vpre_[i_])); }
#define DTA_V_FRAG(S4, DB) (((DH / 32) * (S4) + (DB) < DTA_V_PRELOAD_N) ? vpre_[(DH / 32) * (S4) + (DB) < DTA_V_PRELOAD_N ? (DH / 32) * (S4) + (DB) : 0] : tr_frag_o<v8>(Vs + 32 * DH * (S4), offs, (DB)))
#else
#define DTA_V_PRELOAD
#define DTA_V_FRAG(S4, DB) tr_frag_o<v8>(Vs + 32 * DH * (S4), offs, (DB))
#endif

// The 16 score MFMAs of a tile.  Default: the two key blocks' chains INTERLEAVED with the fragment reads one k-step ahead (every MFMA's
// operand was requested two MFMAs earlier and consecutive MFMAs do not depend on each other); -DDTA_SCORE_ORDER=0: block after block
// (hipcc then waits for each of the first eight fragment reads right after issuing it).
#ifndef DTA_SCORE_ORDER
#define DTA_SCORE_ORDER 1
#endif
#if DTA_SCORE_ORDER
#define DTA_SCORE_MFMAS                                                                                    \
    { v8 ka_ = *reinterpret_cast<const v8*>(Ks + offs.row[0]), kb2_ = *reinterpret_cast<const v8*>(Ks + 64 * DH + offs.row[0]); \
      _Pragma("unroll") for (int s = 0; s < DH / 16; ++s) {                                                \
        v8 na_ = ka_, nb_ = kb2_;                                                                          \
        if (s < DH / 16 - 1) { na_ = *reinterpret_cast<const v8*>(Ks + offs.row[s + 1]); nb_ = *reinterpret_cast<const v8*>(Ks + 64 * DH + offs.row[s + 1]); } \
        X[0] = T::mma(ka_, qf[s], X[0]); X[1] = T::mma(kb2_, qf[s], X[1]);                                 \
        ka_ = na_; kb2_ = nb_;                                                                             \
      } }
#else
#define DTA_SCORE_MFMAS                                                                                    \
    _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                                       \
      _Pragma("unroll") for (int s = 0; s < DH / 16; ++s)                                                  \
        X[kb] = T::mma(*reinterpret_cast<const v8*>(Ks + 64 * DH * kb + offs.row[s]), qf[s], X[kb]);
#endif

// =================================================================================================
// forward.  HPB = query heads of one kv group handled by a workgroup (waves 4*hb .. 4*hb+3 own head hb);
// they share the staged K/V tiles.  One barrier per 64-key tile, LDS double buffered, tile loop unrolled
// over the two buffers so that every LDS address is lane-offset + immediate.
// =================================================================================================
template <int DT, int HPB, int DH, bool WIN, bool CAP>
__global__ __launch_bounds__(256 * HPB, 2) void tree_attn_fwd_kernel(AttnP<WIN, CAP> p) {
  using T = Ty<DT>; using e = typename T::e; using v8 = typename T::v8; using v4 = typename T::v4;
  constexpr int TB = tile_bytes<DH>(), NKS = DH / 16, NDB = DH / 32;      // image bytes, k-steps over D, 32-wide accumulator blocks over D
  constexpr int NW = 4 * HPB, BUF = 2 * TB + SE_BYTES;
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);        // wave-uniform values live in SGPRs
  const int hb = wave >> 2, rw = wave & 3;
  const int bid = blockIdx.x;
  const int hgroups = p.hgroups;
  const int kvh = bid % p.Hkv; const int rest = bid / p.Hkv; const int hgb = rest % hgroups;
  const int nqt = (p.Tq + DTA_QTILE - 1) / DTA_QTILE;
  const int qt = nqt - 1 - rest / hgroups;                          // deepest (heaviest) query tiles first
  const int hq = kvh * p.group + p.head0 + hgb * HPB + hb;
  const int q0 = qt * DTA_QTILE;
  const int qrow = q0 + rw * 32 + r;
  const int qrow_c = qrow < p.Tq ? qrow : p.Tq - 1;
  const int qidx = p.q_offset + qrow;
  // window: wlo = this row's lowest visible key; wmax = the largest such bound over the tile in the stack form (keys below it need the
  // mask; the packed form's runs carry that flag from the windowed plan)
  int wlo = 0, wmax = 0;
  if constexpr (WIN) {
    wlo = p.win_lo ? p.win_lo[qrow_c] : (qidx - p.window + 1 > 0 ? qidx - p.window + 1 : 0);
    wmax = p.win_lo ? 0 : p.q_offset + (q0 + DTA_QTILE < p.Tq ? q0 + DTA_QTILE : p.Tq) - p.window;
  }

  TileIter it; it.runs = p.runs; it.diag_first_q = p.subtree_end ? -64 : p.q_offset + q0;
  if (p.runs) { it.ri = p.run_ptr[qt]; it.re = p.run_ptr[qt + 1]; if (!it.load_run()) return; }
  else { it.ri = 0; it.re = 1; it.k0 = 0; it.flag = 1; int last = p.q_offset + (q0 + DTA_QTILE < p.Tq ? q0 + DTA_QTILE : p.Tq); it.kend = last < p.Tk ? last : p.Tk; if (it.kend <= 0) return; }
  if constexpr (WIN) {                     // stack form: nothing below the first row's bound is visible to the tile
    const int lo0 = p.q_offset + q0 - p.window + 1;
    if (!p.runs && !p.win_lo && lo0 > 0) { it.k0 = lo0; if (it.k0 >= it.kend) return; }
  }

  const e* qp = reinterpret_cast<const e*>(p.q) + (int64_t)qrow_c * p.q_st + (int64_t)hq * p.q_sh;
  v8 qf[NKS];
#pragma unroll
  for (int s = 0; s < NKS; ++s) qf[s] = *reinterpret_cast<const v8*>(qp + 16 * s + 8 * h);

  const e* kbase = reinterpret_cast<const e*>(p.k) + (int64_t)kvh * p.kv_sh;
  const e* vbase = reinterpret_cast<const e*>(p.v) + (int64_t)kvh * p.v_sh;
  const FragOffsT<DH> offs = frag_offsets<DH>(lane);
  DTA_KV_OFFSETS(NW)

  f32x16 O[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int g = 0; g < 16; ++g) O[db][g] = 0.f;
  float m = -1e30f, lsum = 0.f;
  DTA_CAP_CONSTANTS

  int ck0 = it.k0, ckend = it.kend; bool cmask = it.masked() || (WIN && it.k0 < wmax);
  DTA_KV_DMA(smem, it.k0, NW)
  bool has_next = it.advance();
  // The Q fragments must be COMPLETE in hipcc's own book-keeping before the loop: it cannot see the asm DMA, but it does count the plain
  // global loads of Q, and with them still "pending" at the loop header it put `s_waitcnt vmcnt(7) .. vmcnt(0)` in front of the first eight
  // score MFMAs of the loop body - where vmcnt(0) also waits for the NEXT tile's DMA issued a few hundred cycles earlier.
#pragma unroll
  for (int s = 0; s < NKS; ++s) asm volatile("" : "+v"(qf[s]));
  DMA_WAIT(); __syncthreads();

  // one tile out of buffer BUFI (compile-time): prefetch the next tile into the other buffer, S^T, softmax, PV
#define FWD_TILE(BUFI)                                                                                     \
  {                                                                                                        \
    int nk0_ = 0, nkend_ = 0; bool nmask_ = false;                                                         \
    DTA_STAMP_AT(5) DTA_STAMP_TILE                                                                         \
    if (has_next) { nk0_ = it.k0; nkend_ = it.kend; nmask_ = it.masked() || (WIN && it.k0 < wmax); DTA_KV_DMA(smem + (1 - (BUFI)) * BUF, it.k0, NW) } \
    DTA_STAMP_AT(0)                                                                                        \
    const char* Ks = smem + (BUFI) * BUF; const char* Vs = Ks + TB;                                \
    const int* se_s = reinterpret_cast<const int*>(Ks + 2 * TB);                                   \
    f32x16 X[2];                                                                                           \
    _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                                       \
      _Pragma("unroll") for (int g = 0; g < 16; ++g) X[kb][g] = 0.f;                                       \
    DTA_SCORE_MFMAS                                                                                        \
    if constexpr (CAP) {                         /* X := tanh(scale q.k / softcap), before the mask; c carries the softcap */ \
      _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                                     \
        _Pragma("unroll") for (int g = 0; g < 16; ++g) X[kb][g] = cap_tanh(X[kb][g] * kcap);                 \
    }                                                                                                      \
    DTA_STAMP_AT(1)                                                                                        \
    if (cmask) {                                                                                           \
      const int qlim = qidx < ckend ? qidx : ckend - 1;      /* keys at or beyond the run end never count */ \
      _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                                     \
        _Pragma("unroll") for (int gq = 0; gq < 4; ++gq) {                                                 \
          const int kl = 32 * kb + 8 * gq + 4 * h;                                                         \
          const int4 se4 = *reinterpret_cast<const int4*>(se_s + kl);                                      \
          const int sev[4] = {se4.x, se4.y, se4.z, se4.w};                                                 \
          _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                  \
            const bool ok = (ck0 + kl + j <= qlim) && (qidx < sev[j]) && (!WIN || ck0 + kl + j >= wlo);    \
            X[kb][4 * gq + j] = ok ? X[kb][4 * gq + j] : -INFINITY;                                        \
          }                                                                                                \
        }                                                                                                  \
    }                                                                                                      \
    DTA_V_PRELOAD                                                                                          \
    float mx = max3(X[0][0], X[0][1], X[0][2]), mx1 = max3(X[1][0], X[1][1], X[1][2]);   /* two independent chains */ \
    _Pragma("unroll") for (int g = 3; g < 15; g += 2) { mx = max3(mx, X[0][g], X[0][g + 1]); mx1 = max3(mx1, X[1][g], X[1][g + 1]); } \
    mx = max3(mx, X[0][15], mx1);                                                                          \
    mx = half_max(fmaxf(mx, X[1][15]));        /* v_permlane32_swap: no LDS round trip (ds_bpermute + 6 address instructions before) */ \
    const float mc = mx * c;                                                                               \
    if (__any(mc > m + FWD_THR)) {             /* O is rescaled only when some row's maximum grew by more than the deferral threshold */ \
      const float mnew = fmaxf(m, mc);                                                                     \
      const float alpha = fast_exp2(m - mnew);                                                             \
      m = mnew; lsum *= alpha;                                                                             \
      _Pragma("unroll") for (int db = 0; db < NDB; ++db)                                                   \
        _Pragma("unroll") for (int g = 0; g < 16; ++g) O[db][g] *= alpha;                                  \
    }                                                                                                      \
    DTA_STAMP_AT(2)                                                                                        \
    _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                                       \
      _Pragma("unroll") for (int g = 0; g < 16; ++g) { const float pv = fast_exp2(__builtin_fmaf(X[kb][g], c, -m)); lsum += pv; X[kb][g] = pv; } \
    _Pragma("unroll") for (int s4 = 0; s4 < 4; ++s4) {                                                     \
      const v8 pb = pack_half<DT>(X[s4 >> 1], s4 & 1);                                                     \
      _Pragma("unroll") for (int db = 0; db < NDB; ++db) O[db] = T::mma(DTA_V_FRAG(s4, db), pb, O[db]);      \
    }                                                                                                      \
    DTA_STAMP_AT(3)                                                                                        \
    DMA_WAIT(); __syncthreads();               /* the next tile has landed in every wave's view */          \
    DTA_STAMP_AT(4)                                                                                        \
    if (!has_next) break;                                                                                  \
    ck0 = nk0_; ckend = nkend_; cmask = nmask_;                                                            \
    has_next = it.advance();                                                                               \
  }
  DTA_STAMP_DECL
  while (true) {
    FWD_TILE(0)
    FWD_TILE(1)
  }
#undef FWD_TILE
  DTA_STAMP_STORE

  lsum += __shfl_xor(lsum, 32);
  const float inv = 1.f / lsum;
  if (qrow < p.Tq) {
    e* op = reinterpret_cast<e*>(p.out) + (int64_t)qrow * p.o_st + (int64_t)hq * p.o_sh;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        v4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = (e)(O[db][4 * gq + j] * inv);
        *reinterpret_cast<v4*>(op + 32 * db + 8 * gq + 4 * h) = w;
      }
    if (h == 0) p.lse_w[(int64_t)hq * p.Tq + qrow] = m + __builtin_amdgcn_logf(lsum);   // v_log_f32 = log2
  }
}

// =================================================================================================
// backward part 1: delta + dQ   (query tile owns the workgroup; same sweep as the forward)
// =================================================================================================
template <int DT, int HPB, int DH, bool WIN, bool CAP>
__global__ __launch_bounds__(256 * HPB, 2) void tree_attn_bwd_dq_kernel(AttnP<WIN, CAP> p) {
  using T = Ty<DT>; using e = typename T::e; using v8 = typename T::v8; using v4 = typename T::v4;
  constexpr int TB = tile_bytes<DH>(), NKS = DH / 16, NDB = DH / 32;
  __shared__ __attribute__((aligned(16))) char smem[2 * (2 * TB + SE_BYTES)];

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);        // wave-uniform values live in SGPRs
  const int hb = wave >> 2, rw = wave & 3;
  const int bid = blockIdx.x;
  const int hgroups = p.hgroups;
  const int kvh = bid % p.Hkv; const int rest = bid / p.Hkv; const int hgb = rest % hgroups;
  const int nqt = (p.Tq + DTA_QTILE - 1) / DTA_QTILE;
  const int qt = nqt - 1 - rest / hgroups;
  const int hq = kvh * p.group + p.head0 + hgb * HPB + hb;
  const int q0 = qt * DTA_QTILE;
  const int qrow = q0 + rw * 32 + r;
  const int qrow_c = qrow < p.Tq ? qrow : p.Tq - 1;
  const int qidx = p.q_offset + qrow;
  // window: wlo = this row's lowest visible key; wmax = the largest such bound over the tile in the stack form (keys below it need the
  // mask; the packed form's runs carry that flag from the windowed plan)
  int wlo = 0, wmax = 0;
  if constexpr (WIN) {
    wlo = p.win_lo ? p.win_lo[qrow_c] : (qidx - p.window + 1 > 0 ? qidx - p.window + 1 : 0);
    wmax = p.win_lo ? 0 : p.q_offset + (q0 + DTA_QTILE < p.Tq ? q0 + DTA_QTILE : p.Tq) - p.window;
  }

  const e* qp = reinterpret_cast<const e*>(p.q) + (int64_t)qrow_c * p.q_st + (int64_t)hq * p.q_sh;
  const e* dop = reinterpret_cast<const e*>(p.dout) + (int64_t)qrow_c * p.o_st + (int64_t)hq * p.o_sh;
  const e* op = reinterpret_cast<const e*>(p.o) + (int64_t)qrow_c * p.o_st + (int64_t)hq * p.o_sh;
  v8 qf[NKS], dof[NKS];
  float dsum = 0.f;
#pragma unroll
  for (int s = 0; s < NKS; ++s) {
    qf[s] = *reinterpret_cast<const v8*>(qp + 16 * s + 8 * h);
    dof[s] = *reinterpret_cast<const v8*>(dop + 16 * s + 8 * h);
    const v8 of = *reinterpret_cast<const v8*>(op + 16 * s + 8 * h);
#pragma unroll
    for (int j = 0; j < 8; ++j) dsum += (float)dof[s][j] * (float)of[j];
  }
  dsum += __shfl_xor(dsum, 32);
  const float delta = dsum;
  const float lse2 = p.lse_r[(int64_t)hq * p.Tq + qrow_c];
  if (h == 0 && qrow < p.Tq) p.delta[(int64_t)hq * p.Tq + qrow] = -delta;    // workspace holds -delta: the dK/dV kernel loads it as the INITIAL dP accumulator

  TileIter it; it.runs = p.runs; it.diag_first_q = p.subtree_end ? -64 : p.q_offset + q0;
  bool any = true;
  if (p.runs) { it.ri = p.run_ptr[qt]; it.re = p.run_ptr[qt + 1]; any = it.load_run(); }
  else { it.ri = 0; it.re = 1; it.k0 = 0; it.flag = 1; int last = p.q_offset + (q0 + DTA_QTILE < p.Tq ? q0 + DTA_QTILE : p.Tq); it.kend = last < p.Tk ? last : p.Tk; any = it.kend > 0; }
  if constexpr (WIN) {                     // stack form: nothing below the first row's bound is visible to the tile
    const int lo0 = p.q_offset + q0 - p.window + 1;
    if (!p.runs && !p.win_lo && lo0 > 0) { it.k0 = lo0; any = any && it.k0 < it.kend; }
  }

  const e* kbase = reinterpret_cast<const e*>(p.k) + (int64_t)kvh * p.kv_sh;
  const e* vbase = reinterpret_cast<const e*>(p.v) + (int64_t)kvh * p.v_sh;
  constexpr int NW = 4 * HPB, BUF = 2 * TB + SE_BYTES;
  DTA_KV_OFFSETS(NW)                      // K/V tiles by LDS-DMA as in the forward (no staging registers, no ds_write)

  f32x16 DQ[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int g = 0; g < 16; ++g) DQ[db][g] = 0.f;
  DTA_CAP_CONSTANTS

  // dP starts at -delta (this lane's query row) instead of 0: dS/scale = p * dP' costs one multiply per element, and the softmax
  // scale goes onto dQ once, in the epilogue (as the dK/dV kernel does for dK)
  f32x16 DI;
#pragma unroll
  for (int g = 0; g < 16; ++g) DI[g] = -delta;
  if (any) {
    int ck0 = it.k0, ckend = it.kend; bool cmask = it.masked() || (WIN && it.k0 < wmax);
    DTA_KV_DMA(smem, it.k0, NW)
    bool has_next = it.advance();
    DMA_WAIT(); __syncthreads();
    int cur = 0;
    while (true) {
      int nk0 = 0, nkend = 0; bool nmask = false;
      if (has_next) { nk0 = it.k0; nkend = it.kend; nmask = it.masked() || (WIN && it.k0 < wmax); DTA_KV_DMA(smem + (cur ^ 1) * BUF, it.k0, NW) }
      const char* Ks = smem + cur * BUF; const char* Vs = Ks + TB;
      const int* se_s = reinterpret_cast<const int*>(Ks + 2 * TB);
      // one 32-key block at a time keeps S^T/dP^T at 32 live accumulators (2 waves per SIMD need <= 256 registers)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        f32x16 X, DP;
#pragma unroll
        for (int g = 0; g < 16; ++g) X[g] = 0.f;
        {                                                  // fragment reads one k-step ahead of the MFMAs that use them
          v8 kf_ = row_frag<v8, DH>(Ks, 32 * kb + r, h), vf_ = row_frag<v8, DH>(Vs, 32 * kb + r, h);
#pragma unroll
          for (int s = 0; s < NKS; ++s) {
            v8 nk_ = kf_, nv_ = vf_;
            if (s < NKS - 1) { nk_ = row_frag<v8, DH>(Ks, 32 * kb + r, 2 * s + 2 + h); nv_ = row_frag<v8, DH>(Vs, 32 * kb + r, 2 * s + 2 + h); }
            X = T::mma(kf_, qf[s], X);
            DP = T::mma(vf_, dof[s], s == 0 ? DI : DP);
            kf_ = nk_; vf_ = nv_;
          }
          // hipcc's scheduler otherwise sinks every read pair directly in front of its two MFMAs (one register pair re-used: each MFMA
          // pair then waits a full LDS latency): pin the order {4 reads} {2 MFMA, 2 reads} x (NKS - 2) {4 MFMA}
          __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
          for (int i_ = 0; i_ < NKS - 2; ++i_) { __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); __builtin_amdgcn_sched_group_barrier(0x100, 2, 0); }
          __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        }
        // dS^T / scale = P ∘ (dP − delta); the interval mask only on tiles of runs flagged partial
        // CAP: t = tanh(z / softcap) stands for the score and dz / scale = p (dP − delta)(1 − t²), one element at a time (a separate pass
        // over the 16 scores kept t and 1 − t² live beside X and DP: 256 registers and a spill in the windowed D = 128 form)
        if (cmask) {
          const int qlim = qidx < ckend ? qidx : ckend - 1;      // keys at or beyond the run end never count
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) {
            const int kl = 32 * kb + 8 * gq + 4 * h;
            const int4 se4 = *reinterpret_cast<const int4*>(se_s + kl);
            const int sev[4] = {se4.x, se4.y, se4.z, se4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int g = 4 * gq + j;
              const bool ok = (ck0 + kl + j <= qlim) && (qidx < sev[j]) && (!WIN || ck0 + kl + j >= wlo);
              if constexpr (CAP) {
                const float t = cap_tanh(X[g] * kcap);
                const float pv = ok ? fast_exp2(__builtin_fmaf(t, c, -lse2)) : 0.f;
                X[g] = pv * DP[g] * __builtin_fmaf(-t, t, 1.f);
              } else {
              const float pv = ok ? fast_exp2(__builtin_fmaf(X[g], c, -lse2)) : 0.f;
              X[g] = pv * DP[g];
              }
            }
          }
        } else {
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            if constexpr (CAP) { const float t = cap_tanh(X[g] * kcap); X[g] = fast_exp2(__builtin_fmaf(t, c, -lse2)) * DP[g] * __builtin_fmaf(-t, t, 1.f); }
            else X[g] = fast_exp2(__builtin_fmaf(X[g], c, -lse2)) * DP[g];
          }
        }
        // dQ^T[d][q] += K^T · dS^T
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const v8 db_ = pack_half<DT>(X, s2);
#pragma unroll
          for (int db = 0; db < NDB; ++db) DQ[db] = T::mma(tr_frag<v8, DH>(Ks, 32 * kb + 16 * s2, db, lane), db_, DQ[db]);
        }
      }
      DMA_WAIT(); __syncthreads();
      if (!has_next) break;
      cur ^= 1; ck0 = nk0; ckend = nkend; cmask = nmask;
      has_next = it.advance();
    }
  }
  if (qrow < p.Tq) {
    e* dqp = reinterpret_cast<e*>(p.dq) + (int64_t)qrow * p.dq_st + (int64_t)hq * p.dq_sh;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        v4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = (e)(DQ[db][4 * gq + j] * p.scale);
        *reinterpret_cast<v4*>(dqp + 32 * db + 8 * gq + 4 * h) = w;
      }
  }
}

// =================================================================================================
// backward part 2: dK, dV.  Key tile owns the workgroup.
// =================================================================================================
// -------------------------------------------------------------------------------------------------
// dK/dV with TWO waves per SIMD (8 waves): the two wave groups own the same 128 keys and split every 64-row query tile
// between them (group g takes rows 32g..32g+31), so they share ONE double-buffered Q/dO image.  To fit 256 registers
// the K/V fragments (pure MFMA B operands) live in LDS in fragment order (one lane-linear, conflict-free ds_read_b128
// per use) instead of 64 registers.  The groups' partial dK/dV are summed through LDS in a fixed order at the end.
// -------------------------------------------------------------------------------------------------
// dkv2's S / dP chains: left alone (-DDTA_KV2_PIN=0) hipcc runs most of the dP MFMAs and then the S MFMAs as two dependent chains, every operand
// read directly in front of the MFMA that uses it.  Default 2: reads stay just in time but the two chains ALTERNATE (-1.0 %, three alternating
// pairs on one box: 1.3407 -> 1.3272 ms); 1: {delta row + operands of two k-steps} {2 MFMA, 4 reads} x 6 {4 MFMA} - read bursts, 5 spills, 7 % slower.
#ifndef DTA_KV2_PIN
#define DTA_KV2_PIN 2
#endif
#if DTA_KV2_PIN == 2      /* just-in-time reads, but the two chains alternating: {delta row} {2 reads, 1 MFMA} x 16 */
#define DTA_KV2_PIN_ORDER                                                                                  \
    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);                                                     \
    _Pragma("unroll") for (int i_ = 0; i_ < 2 * NKS; ++i_) { __builtin_amdgcn_sched_group_barrier(0x100, 2, 0); __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); }
#elif DTA_KV2_PIN
#define DTA_KV2_PIN_ORDER                                                                                  \
    __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);                                                    \
    _Pragma("unroll") for (int i_ = 0; i_ < NKS - 2; ++i_) { __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); __builtin_amdgcn_sched_group_barrier(0x100, 4, 0); } \
    __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
#else
#define DTA_KV2_PIN_ORDER
#endif

template <int D> constexpr int kv2_slot() { return 2 * (D / 16) * 1024; }    // one key slot: {K: D/16 fragments x 1 KiB, V: D/16 x 1 KiB}
template <int D> constexpr int kv2_frags() { return 4 * kv2_slot<D>(); }    // 4 key slots
template <int D, bool WIN> constexpr int kv2_buf() { return 2 * tile_bytes<D>() + (WIN ? 768 : 512); }   // + row constants lse, -delta (, win_lo)
template <int D, bool WIN> constexpr int kv2_lds() { return kv2_frags<D>() + 2 * kv2_buf<D, WIN>() + 16; }   // + se_min[4]: ONE __shared__ object (a second one makes hipcc drain vmcnt in front of every LDS read)

template <int DT, int DH, bool WIN, bool CAP>
__global__ __launch_bounds__(512, 2) void tree_attn_bwd_dkv2_kernel(AttnP<WIN, CAP> p) {
  using T = Ty<DT>; using e = typename T::e; using v8 = typename T::v8; using v4 = typename T::v4;
  constexpr int KT = 128;
  constexpr int TB = tile_bytes<DH>(), NKS = DH / 16, NDB = DH / 32, KV2_FRAGS = kv2_frags<DH>(), KV2_BUF = kv2_buf<DH, WIN>(), KSLOT = kv2_slot<DH>();
  __shared__ __attribute__((aligned(16))) char smem_all[kv2_lds<DH, WIN>()];
  const int tid8 = threadIdx.x, tid = tid8 & 255, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wave8 = __builtin_amdgcn_readfirstlane(tid8 >> 6);       // 0..7
  const int grp = wave8 >> 2, wave = wave8 & 3;
  char* kvs = smem_all + wave * KSLOT;                               // this key slot's K fragments (+KSLOT/2: V)
  char* smem = smem_all + KV2_FRAGS;                                 // the Q/dO buffers
  const int bid = blockIdx.x;
  const int kvh = bid % p.Hkv; const int unit = bid / p.Hkv;
  const int kt = p.dkv_units ? p.dkv_units[4 * unit] : unit;
  const int slab = p.dkv_units ? p.dkv_units[4 * unit + 3] : -1;
  const int k0 = kt * KT;
  const int q_hi = p.q_offset + p.Tq;
  const int kidx = k0 + wave * 32 + r;
  int se_l;
  { const int kc = kidx < p.Tk ? kidx : p.Tk - 1;
    int se = (kidx < p.Tk) ? (p.subtree_end ? p.subtree_end[kidx] : 0x7fffffff) : 0;
    se_l = se < q_hi ? se : q_hi;
    if (grp == 0) {                                                  // group 0 stages the fragments both groups read
      const e* kp = reinterpret_cast<const e*>(p.k) + (int64_t)kc * p.kv_st + (int64_t)kvh * p.kv_sh;
      const e* vp = reinterpret_cast<const e*>(p.v) + (int64_t)kc * p.v_st + (int64_t)kvh * p.v_sh;
#pragma unroll
      for (int s = 0; s < NKS; ++s) {
        *reinterpret_cast<v8*>(kvs + s * 1024 + lane * 16) = *reinterpret_cast<const v8*>(kp + 16 * s + 8 * h);
        *reinterpret_cast<v8*>(kvs + KSLOT / 2 + s * 1024 + lane * 16) = *reinterpret_cast<const v8*>(vp + 16 * s + 8 * h);
      }
    } }
  int* se_min_s = reinterpret_cast<int*>(smem_all + KV2_FRAGS + 2 * KV2_BUF);
  { int mn = se_l;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(mn, o); mn = t < mn ? t : mn; }
    if (lane == 0 && grp == 0) se_min_s[wave] = mn; }
  __syncthreads();
  const int se_min = __builtin_amdgcn_readfirstlane(min(min(se_min_s[0], se_min_s[1]), min(se_min_s[2], se_min_s[3])));

  const FragOffsT<DH> offs = frag_offsets<DH>(lane);
  f32x16 DK[NDB], DV[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int g = 0; g < 16; ++g) { DK[db][g] = 0.f; DV[db][g] = 0.f; }

  int qbeg, qend;
  if (p.dkv_units) { qbeg = __builtin_amdgcn_readfirstlane(p.dkv_units[4 * unit + 1]); qend = __builtin_amdgcn_readfirstlane(p.dkv_units[4 * unit + 2]); }
  else {
    qbeg = k0 > p.q_offset ? k0 : p.q_offset;
    qend = p.ktile_qend ? p.ktile_qend[kt] : q_hi; qend = qend < q_hi ? qend : q_hi;
    if constexpr (WIN) if (!p.win_lo) {          // stack form: query q sees the tile only while q - window + 1 <= its last key
      const int64_t wl = (int64_t)k0 + KT - 1 + p.window; qend = wl < qend ? (int)wl : qend;
    }
  }
  const int ntile = qend > qbeg ? (qend - qbeg + 63) / 64 : 0;
  const int total = ntile * p.group;
  DTA_CAP_CONSTANTS

  // tile DMA: DH/8 one-KiB pieces per image over 8 waves = NP = DH/64 per wave per image (D = 128: piece = 2*wave8 + i, rows 8*wave8 + 4*i ..;
  // D = 64: piece = wave8, rows 8*wave8 ..); lse / delta rows (64 floats each) by 4-byte DMA from waves 0 / 1.
  constexpr int NP = DH / 64;
  uint32_t voff_q[NP], voff_d[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int row_ = 8 * wave8 + (512 / DH) * i + (lane >> dma_lane_row_shift<DH>());
    voff_q[i] = dma_src_off_d<DH>(row_, row_, lane, p.q_st, sizeof(e));
    voff_d[i] = dma_src_off_d<DH>(row_, row_, lane, p.o_st, sizeof(e));
  }
  const uint32_t lds_tiles = lds_addr(smem);
  // scalar cursor of the NEXT tile to stage: byte offsets of its first row in q / dout and float offset of its row
  // constants; advanced by additions (64 rows down, or to row qbeg of the next query head) - no 64-bit multiplies per tile
  const int64_t q_step = 64 * p.q_st * (int64_t)sizeof(e), d_step = 64 * p.o_st * (int64_t)sizeof(e);
  const int64_t q_wrap = p.q_sh * (int64_t)sizeof(e) - ntile * q_step, d_wrap = p.o_sh * (int64_t)sizeof(e) - ntile * d_step;
  int64_t q_cur = ((int64_t)(kvh * p.group) * p.q_sh + (int64_t)(qbeg - p.q_offset) * p.q_st) * (int64_t)sizeof(e);
  int64_t d_cur = ((int64_t)(kvh * p.group) * p.o_sh + (int64_t)(qbeg - p.q_offset) * p.o_st) * (int64_t)sizeof(e);
  int64_t c_cur = (int64_t)(kvh * p.group) * p.Tq;
  int row_n = qbeg - p.q_offset, ti_n = 0;
#define KV2_DMA(B)                                                                                         \
  { const uint32_t lb_ = lds_tiles + (uint32_t)(B) * KV2_BUF;                                              \
    if (wave8 < 2) { int qr_ = row_n + lane; qr_ = qr_ < p.Tq ? qr_ : p.Tq - 1;   /* wave 0: lse[64], wave 1: delta[64] */ \
      dma_dword((uint32_t)qr_ * 4u, (wave8 == 0 ? p.lse_r : p.delta) + c_cur, lb_ + 2 * TB + wave8 * 256); } \
    if constexpr (WIN) if (wave8 == 2 && p.win_lo) { int qr_ = row_n + lane; qr_ = qr_ < p.Tq ? qr_ : p.Tq - 1;   /* wave 2: win_lo[64] */ \
      dma_dword((uint32_t)qr_ * 4u, p.win_lo, lb_ + 2 * TB + 512); }                                       \
    uint32_t oq_[NP], od_[NP];                                                                             \
    _Pragma("unroll") for (int i_ = 0; i_ < NP; ++i_) { oq_[i_] = voff_q[i_]; od_[i_] = voff_d[i_]; }      \
    if (row_n + 64 > p.Tq) {                       /* ragged last tile of the tensor: clamp the row per lane */ \
      _Pragma("unroll") for (int i_ = 0; i_ < NP; ++i_) {                                                  \
        const int ra_ = 8 * wave8 + (512 / DH) * i_ + (lane >> dma_lane_row_shift<DH>());                  \
        const int ca_ = row_n + ra_ < p.Tq ? ra_ : p.Tq - 1 - row_n;                                       \
        oq_[i_] = dma_src_off_d<DH>(ca_, ra_, lane, p.q_st, sizeof(e)); od_[i_] = dma_src_off_d<DH>(ca_, ra_, lane, p.o_st, sizeof(e)); } } \
    if constexpr (NP == 2) dma_pair2(oq_[0], oq_[1], reinterpret_cast<const char*>(p.q) + q_cur, od_[0], od_[1], reinterpret_cast<const char*>(p.dout) + d_cur, lb_ + wave8 * 2048); \
    else dma_one2<TB>(oq_[0], reinterpret_cast<const char*>(p.q) + q_cur, od_[0], reinterpret_cast<const char*>(p.dout) + d_cur, lb_ + wave8 * 1024); \
    ++ti_n; row_n += 64; q_cur += q_step; d_cur += d_step;                                                 \
    if (ti_n >= ntile) { ti_n = 0; row_n = qbeg - p.q_offset; q_cur += q_wrap; d_cur += d_wrap; c_cur += p.Tq; } }

  // Per-lane LDS byte offsets of every fragment read of this wave group inside a tile buffer, computed once; the tile loop is
  // unrolled over the two buffers so that the buffer offset is an instruction immediate (no per-tile address VALU).
  int ar[NKS], at[NKS];
#pragma unroll
  for (int j = 0; j < NKS; ++j) { ar[j] = offs.row[j] + grp * (64 * DH); at[j] = offs.tr[j] + grp * (64 * DH); }
  const int rc_off = (32 * grp + 4 * h) * 4;                            // this lane's first row constant (lse / -delta) inside a buffer

  // one 64-row query tile out of buffer BUFI (compile-time)
#define KV2_TILE(BUFI)                                                                                     \
  {                                                                                                        \
    const int ti = ti_c;                                                                                   \
    ti_c += 1;                                                                                             \
    if (ti_c >= ntile) ti_c = 0;                                                                           \
    if (idx + 1 < total) KV2_DMA(1 - (BUFI))      /* lands while this tile computes; waited for at the tile end */ \
    const char* tb = smem + (BUFI) * KV2_BUF;                                                              \
    const char* rc = tb + 2 * TB + rc_off;                                                         \
    const int qi0 = qbeg + 64 * ti + 32 * grp;                       /* packed index of this group's first row */ \
    bool full = (qbeg + 64 * ti >= k0 + KT - 1) && (qbeg + 64 * ti + 63 < se_min);   /* workgroup-uniform: no mask needed */ \
    if constexpr (WIN) full = full && !p.win_lo && qbeg + 64 * ti + 64 - p.window <= k0;   /* window: stack form only */ \
    /* S starts at 0 (inline constant); dP starts at -delta, read from LDS straight into the accumulator registers:    \
       p = exp2(c*S - lse),  dS/scale = p * dP'  with dP' = dO.V^T - delta  (the softmax scale of dS goes onto dK once, in the epilogue) */ \
    f32x16 S, DP;                                                                                          \
    _Pragma("unroll") for (int gq = 0; gq < 4; ++gq) {                                                     \
      const float4 d4 = *reinterpret_cast<const float4*>(rc + 256 + 32 * gq);                              \
      DP[4 * gq] = d4.x; DP[4 * gq + 1] = d4.y; DP[4 * gq + 2] = d4.z; DP[4 * gq + 3] = d4.w;              \
    }                                                                                                      \
    _Pragma("unroll") for (int g = 0; g < 16; ++g) S[g] = 0.f;                                             \
    _Pragma("unroll") for (int s = 0; s < NKS; ++s) {                                                      \
      const v8 aq = *reinterpret_cast<const v8*>(tb + ar[s]);                                              \
      const v8 ad = *reinterpret_cast<const v8*>(tb + ar[s] + TB);                                         \
      const v8 kfs = *reinterpret_cast<const v8*>(kvs + s * 1024 + lane * 16);                             \
      const v8 vfs = *reinterpret_cast<const v8*>(kvs + KSLOT / 2 + s * 1024 + lane * 16);                 \
      S = T::mma(aq, kfs, S); DP = T::mma(ad, vfs, DP);                                                    \
    }                                                                                                      \
    DTA_KV2_PIN_ORDER                                                                                      \
    float nl[16];                                                                                          \
    _Pragma("unroll") for (int gq = 0; gq < 4; ++gq) {                                                     \
      const float4 l4 = *reinterpret_cast<const float4*>(rc + 32 * gq);                                    \
      nl[4 * gq] = l4.x; nl[4 * gq + 1] = l4.y; nl[4 * gq + 2] = l4.z; nl[4 * gq + 3] = l4.w;              \
    }                                                                                                      \
    if constexpr (CAP) {                           /* S := t = tanh(z / softcap); DP := (dP - delta)(1 - t^2): dz / scale = p * DP */ \
      _Pragma("unroll") for (int g = 0; g < 16; ++g) { const float t = cap_tanh(S[g] * kcap); S[g] = t; DP[g] *= __builtin_fmaf(-t, t, 1.f); } \
    }                                                                                                      \
    if (full) {                                                                                            \
      _Pragma("unroll") for (int g = 0; g < 16; ++g) {                                                     \
        const float pv = fast_exp2(__builtin_fmaf(S[g], c, -nl[g]));                                       \
        S[g] = pv;                                                                                         \
        DP[g] = pv * DP[g];                                                                                \
      }                                                                                                    \
    } else {                                                                                               \
      int wl[16];                                   /* window: each row's lowest visible key (staged row constant / stack form) */ \
      if constexpr (WIN) {                                                                                 \
        if (p.win_lo) {                                                                                    \
          _Pragma("unroll") for (int gq = 0; gq < 4; ++gq) {                                               \
            const int4 w4 = *reinterpret_cast<const int4*>(rc + 512 + 32 * gq);                            \
            wl[4 * gq] = w4.x; wl[4 * gq + 1] = w4.y; wl[4 * gq + 2] = w4.z; wl[4 * gq + 3] = w4.w; }      \
        } else {                                                                                           \
          _Pragma("unroll") for (int g = 0; g < 16; ++g) wl[g] = qi0 + 8 * (g >> 2) + 4 * h + (g & 3) - p.window + 1; } \
      }                                                                                                    \
      _Pragma("unroll") for (int g = 0; g < 16; ++g) {                                                     \
        const int qi = qi0 + 8 * (g >> 2) + 4 * h + (g & 3);                                               \
        const bool ok = (kidx <= qi) && (qi < se_l) && (!WIN || kidx >= wl[g]);                            \
        const float pv = ok ? fast_exp2(__builtin_fmaf(S[g], c, -nl[g])) : 0.f;                            \
        S[g] = pv;                                                                                         \
        DP[g] = pv * DP[g];                                                                                \
      }                                                                                                    \
    }                                                                                                      \
    _Pragma("unroll") for (int s2 = 0; s2 < 2; ++s2) {                                                     \
      const v8 pb = pack_half<DT>(S, s2), sbf = pack_half<DT>(DP, s2);                                     \
      _Pragma("unroll") for (int db = 0; db < NDB; ++db) {                                                 \
        const v8 adt = tr_pair<v8>(tb + at[db] + TB + 32 * DH * s2, tb + at[NDB + db] + TB + 32 * DH * s2); \
        const v8 aqt = tr_pair<v8>(tb + at[db] + 32 * DH * s2, tb + at[NDB + db] + 32 * DH * s2);          \
        DV[db] = T::mma(adt, pb, DV[db]); DK[db] = T::mma(aqt, sbf, DK[db]);                               \
      }                                                                                                    \
    }                                                                                                      \
    DMA_WAIT(); __syncthreads();                                                                           \
    ++idx;                                                                                                 \
  }

  {
    int ti_c = 0;
    if (total > 0) KV2_DMA(0)
    DMA_WAIT(); __syncthreads();
    int idx = 0;
    while (idx < total) {
      KV2_TILE(0)
      if (idx >= total) break;
      KV2_TILE(1)
    }
  }
#undef KV2_TILE
#undef KV2_DMA
  {
    // group 1 hands its partial sums to group 0 through LDS, 32 accumulators (one d-block of dK and dV) at a time
    float* red = reinterpret_cast<float*>(smem_all);
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      if (grp == 1) {
#pragma unroll
        for (int g = 0; g < 16; ++g) { red[g * 256 + tid] = DK[db][g]; red[(16 + g) * 256 + tid] = DV[db][g]; }
      }
      __syncthreads();
      if (grp == 0) {
#pragma unroll
        for (int g = 0; g < 16; ++g) { DK[db][g] += red[g * 256 + tid]; DV[db][g] += red[(16 + g) * 256 + tid]; }
      }
      __syncthreads();
    }
    if (grp == 1) return;
  }
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int g = 0; g < 16; ++g) DK[db][g] *= p.scale;
  const int kloc = wave * 32 + r;
  if (slab >= 0) {
    float* ws = p.dkv_ws + ((int64_t)slab * p.Hkv + kvh) * (2 * KT * DH) + (int64_t)kloc * DH;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int d = 32 * db + 8 * gq + 4 * h;
        *reinterpret_cast<float4*>(ws + d) = make_float4(DK[db][4 * gq], DK[db][4 * gq + 1], DK[db][4 * gq + 2], DK[db][4 * gq + 3]);
        *reinterpret_cast<float4*>(ws + KT * DH + d) = make_float4(DV[db][4 * gq], DV[db][4 * gq + 1], DV[db][4 * gq + 2], DV[db][4 * gq + 3]);
      }
  } else if (kidx < p.Tk && p.accumulate == 2) {
    // fp32 accumulation buffers (the grad-KV stack of the block-wise engine: hundreds of adds per row stay exact to fp32)
    float* dkp = reinterpret_cast<float*>(p.dk) + (int64_t)kidx * p.dkv_st + (int64_t)kvh * p.dkv_sh;
    float* dvp = reinterpret_cast<float*>(p.dv) + (int64_t)kidx * p.dkv_st + (int64_t)kvh * p.dkv_sh;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int d = 32 * db + 8 * gq + 4 * h;
        float4 a = *reinterpret_cast<const float4*>(dkp + d), b = *reinterpret_cast<const float4*>(dvp + d);
        a.x += DK[db][4 * gq]; a.y += DK[db][4 * gq + 1]; a.z += DK[db][4 * gq + 2]; a.w += DK[db][4 * gq + 3];
        b.x += DV[db][4 * gq]; b.y += DV[db][4 * gq + 1]; b.z += DV[db][4 * gq + 2]; b.w += DV[db][4 * gq + 3];
        *reinterpret_cast<float4*>(dkp + d) = a;
        *reinterpret_cast<float4*>(dvp + d) = b;
      }
  } else if (kidx < p.Tk) {
    e* dkp = reinterpret_cast<e*>(p.dk) + (int64_t)kidx * p.dkv_st + (int64_t)kvh * p.dkv_sh;
    e* dvp = reinterpret_cast<e*>(p.dv) + (int64_t)kidx * p.dkv_st + (int64_t)kvh * p.dkv_sh;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int d = 32 * db + 8 * gq + 4 * h;
        v4 wk, wv;
        if (p.accumulate) {
          const v4 ok_ = *reinterpret_cast<const v4*>(dkp + d); const v4 ov_ = *reinterpret_cast<const v4*>(dvp + d);
#pragma unroll
          for (int j = 0; j < 4; ++j) { wk[j] = (e)(DK[db][4 * gq + j] + (float)ok_[j]); wv[j] = (e)(DV[db][4 * gq + j] + (float)ov_[j]); }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) { wk[j] = (e)DK[db][4 * gq + j]; wv[j] = (e)DV[db][4 * gq + j]; }
        }
        *reinterpret_cast<v4*>(dkp + d) = wk;
        *reinterpret_cast<v4*>(dvp + d) = wv;
      }
  }
}

// Sums the fp32 slabs of every split key tile in a fixed order and writes dK/dV (bitwise reproducible).
// dkv_splits[s] = {key tile, first slab, number of slabs, 0}.
constexpr int FIN_SPLIT = 8;          // blockIdx.y: each (split key tile, kv head) is summed by 8 workgroups — the sums are load-latency bound
template <int DT, int DH>
__global__ __launch_bounds__(256) void tree_attn_bwd_dkv_finalize_kernel(AttnParams p) {
  using e = typename Ty<DT>::e; using v4 = typename Ty<DT>::v4;
  const int KT = p.ktile;
  const int kvh = blockIdx.x % p.Hkv, sp = blockIdx.x / p.Hkv;
  const int kt = p.dkv_splits[4 * sp], first = p.dkv_splits[4 * sp + 1], n = p.dkv_splits[4 * sp + 2];
  constexpr int Q4 = DH / 4, Q4_SHIFT = DH == 128 ? 5 : 4;             // float4 per D-wide row
  const int per = 2 * KT * Q4 / FIN_SPLIT;                                // float4 indices per workgroup
  const float* ws0 = p.dkv_ws + ((int64_t)first * p.Hkv + kvh) * (2 * KT * DH);
  const int64_t slab_st = (int64_t)p.Hkv * (2 * KT * DH);
  for (int i = blockIdx.y * per + threadIdx.x; i < (blockIdx.y + 1) * per; i += 256) {   // float4 index inside a slab
    const int which = i / (KT * Q4), rem = i - which * KT * Q4;
    const int key = rem >> Q4_SHIFT, d = (rem & (Q4 - 1)) << 2;
    const int kidx = kt * KT + key;
    if (kidx >= p.Tk) continue;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int j = 0;
    for (; j + 4 <= n; j += 4) {                                          // four loads in flight, summed in slab order
      const float4 a0 = *reinterpret_cast<const float4*>(ws0 + (j + 0) * slab_st + (int64_t)i * 4);
      const float4 a1 = *reinterpret_cast<const float4*>(ws0 + (j + 1) * slab_st + (int64_t)i * 4);
      const float4 a2 = *reinterpret_cast<const float4*>(ws0 + (j + 2) * slab_st + (int64_t)i * 4);
      const float4 a3 = *reinterpret_cast<const float4*>(ws0 + (j + 3) * slab_st + (int64_t)i * 4);
      acc.x += a0.x; acc.y += a0.y; acc.z += a0.z; acc.w += a0.w;
      acc.x += a1.x; acc.y += a1.y; acc.z += a1.z; acc.w += a1.w;
      acc.x += a2.x; acc.y += a2.y; acc.z += a2.z; acc.w += a2.w;
      acc.x += a3.x; acc.y += a3.y; acc.z += a3.z; acc.w += a3.w;
    }
    for (; j < n; ++j) {
      const float4 v = *reinterpret_cast<const float4*>(ws0 + j * slab_st + (int64_t)i * 4);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    if (p.accumulate == 2) {
      float* outf = reinterpret_cast<float*>(which ? p.dv : p.dk) + (int64_t)kidx * p.dkv_st + (int64_t)kvh * p.dkv_sh + d;
      float4 o = *reinterpret_cast<const float4*>(outf);
      o.x += acc.x; o.y += acc.y; o.z += acc.z; o.w += acc.w;
      *reinterpret_cast<float4*>(outf) = o;
      continue;
    }
    e* out = reinterpret_cast<e*>(which ? p.dv : p.dk) + (int64_t)kidx * p.dkv_st + (int64_t)kvh * p.dkv_sh + d;
    if (p.accumulate) { const v4 o = *reinterpret_cast<const v4*>(out); acc.x += (float)o[0]; acc.y += (float)o[1]; acc.z += (float)o[2]; acc.w += (float)o[3]; }
    v4 w; w[0] = (e)acc.x; w[1] = (e)acc.y; w[2] = (e)acc.z; w[3] = (e)acc.w;
    *reinterpret_cast<v4*>(out) = w;
  }
}

// kernel parameters of the chosen form from the call's arguments (the forward's backward fields are null); hgroups / head0 are set per launch
template <bool WIN, bool CAP> AttnP<WIN, CAP> kernel_params(const DtaAttnArgs& a) {
  AttnP<WIN, CAP> p{};
  if constexpr (WIN) { p.win_lo = a.win_lo; p.window = a.window; }
  if constexpr (CAP) p.softcap = a.softcap;
  p.q = a.q; p.k = a.k; p.v = a.v; p.o = a.o; p.dout = a.dout; p.out = a.out; p.dq = a.dq; p.dk = a.dk; p.dv = a.dv;
  p.lse_w = a.lse_w; p.lse_r = a.lse_r; p.delta = a.delta;
  p.subtree_end = a.subtree_end; p.run_ptr = a.run_ptr; p.runs = a.runs; p.ktile_qend = a.ktile_qend;
  p.dkv_units = a.dkv_units; p.dkv_splits = a.dkv_splits; p.dkv_ws = a.dkv_ws;
  p.Tq = a.Tq; p.Tk = a.Tk; p.q_offset = a.q_offset; p.Hq = a.Hq; p.Hkv = a.Hkv; p.group = a.Hq / a.Hkv;
  p.q_st = a.q_st; p.q_sh = a.q_sh; p.kv_st = a.kv_st; p.kv_sh = a.kv_sh; p.v_st = a.v_st; p.v_sh = a.v_sh; p.o_st = a.o_st; p.o_sh = a.o_sh;
  p.dq_st = a.dq_st; p.dq_sh = a.dq_sh; p.dkv_st = a.dkv_st; p.dkv_sh = a.dkv_sh; p.scale = a.scale; p.accumulate = a.accumulate;
  p.ktile = DTA_KTILE;
  return p;
}

// f(DT, DH): the call's 16-bit dtype and head_dim as std::integral_constant
template <class F> void with_type(const DtaAttnArgs& a, F&& f) {
  using BF = std::integral_constant<int, DTA_BF16>; using FP = std::integral_constant<int, DTA_F16>;
  using D64 = std::integral_constant<int, 64>; using D128 = std::integral_constant<int, 128>;
  if (a.head_dim == 64) { if (a.dtype == DTA_BF16) f(BF{}, D64{}); else f(FP{}, D64{}); }
  else { if (a.dtype == DTA_BF16) f(BF{}, D128{}); else f(FP{}, D128{}); }
}

template <bool WIN, bool CAP> void launch_fwd(const DtaAttnArgs& a) {
  AttnP<WIN, CAP> p = kernel_params<WIN, CAP>(a);
  const int nqt = (a.Tq + DTA_QTILE - 1) / DTA_QTILE;
  // two query heads of a kv group share the staged K/V tiles (512 threads); an odd group sends its last head through the
  // one-head form in a second launch (Qwen3-14B: 40 query / 8 kv heads = 2 pairs + 1 per group)
  const int npair = p.group / 2;
  if (npair > 0) {
    p.hgroups = npair; p.head0 = 0;
    with_type(a, [&](auto dt, auto dh) {
      hipLaunchKernelGGL((tree_attn_fwd_kernel<decltype(dt)::value, 2, decltype(dh)::value, WIN, CAP>), dim3(nqt * a.Hkv * npair), dim3(512), 0, a.stream, p);
    });
  }
  if (p.group % 2) {
    p.hgroups = 1; p.head0 = p.group - 1;
    with_type(a, [&](auto dt, auto dh) {
      hipLaunchKernelGGL((tree_attn_fwd_kernel<decltype(dt)::value, 1, decltype(dh)::value, WIN, CAP>), dim3(nqt * a.Hkv), dim3(256), 0, a.stream, p);
    });
  }
}

// the backward launches: dQ (head pairs, then the odd head alone), dK/dV, and the slab finalize
template <bool WIN, bool CAP> void launch_bwd(const DtaAttnArgs& a) {
  const AttnP<WIN, CAP> p = kernel_params<WIN, CAP>(a);
  const int nqt = (a.Tq + DTA_QTILE - 1) / DTA_QTILE, nkt = (a.Tk + DTA_KTILE - 1) / DTA_KTILE;
  const int which = a.which;
  const bool fin = ((which & 2) && !(which & 8)) || (which & 4);     // slab finalize: with the dK/dV launch unless bit3, or alone (bit2)
  const int ndkv = a.dkv_units ? a.n_units : nkt;
  const int npair = p.group / 2;                                     // as in the forward: head pairs, then the odd head alone
  AttnP<WIN, CAP> pp = p, ps = p;
  pp.hgroups = npair; pp.head0 = 0; ps.hgroups = 1; ps.head0 = p.group - 1;
  const dim3 gqp(nqt * a.Hkv * (npair > 0 ? npair : 1)), gqs(nqt * a.Hkv);
  with_type(a, [&](auto dt, auto dh) {
    constexpr int DT = decltype(dt)::value, DH = decltype(dh)::value;
    if (which & 1) {
      if (npair > 0) hipLaunchKernelGGL((tree_attn_bwd_dq_kernel<DT, 2, DH, WIN, CAP>), gqp, dim3(512), 0, a.stream, pp);
      if (p.group % 2) hipLaunchKernelGGL((tree_attn_bwd_dq_kernel<DT, 1, DH, WIN, CAP>), gqs, dim3(256), 0, a.stream, ps);
    }
    if (which & 2) hipLaunchKernelGGL((tree_attn_bwd_dkv2_kernel<DT, DH, WIN, CAP>), dim3(ndkv * p.Hkv), dim3(512), 0, a.stream, p);
    if (fin && p.dkv_units && a.n_splits > 0)   // the slab sums do not depend on visibility: one finalize kernel for both forms
      hipLaunchKernelGGL((tree_attn_bwd_dkv_finalize_kernel<DT, DH>), dim3(a.n_splits * p.Hkv, FIN_SPLIT), dim3(256), 0, a.stream, static_cast<const AttnParams&>(p));
  });
}

// Argument checks of both entries in the order dta.h gives the status codes.  The forward's backward fields are null / 0 and pass.
int check_args(const DtaAttnArgs& a, bool bwd) {
  if (a.softcap != a.softcap || a.softcap > 3.0e38f) return DTA_EINVAL;          // a cap <= 0 means no cap
  // sliding window: a win_lo without a window, or a packed trie with a window and no win_lo, is refused
  if (a.window <= 0 ? a.win_lo != nullptr : (a.subtree_end && !a.win_lo)) return DTA_EINVAL;
  if (!a.q || !a.k || !a.v || a.Tq <= 0 || a.Tk <= 0 || a.Hq <= 0 || a.Hkv <= 0 || a.q_offset < 0) return DTA_EINVAL;
  if (bwd ? (!a.o || !a.dout || !a.lse_r || !a.delta || !a.dq || !a.dk || !a.dv) : (!a.out || !a.lse_w)) return DTA_EINVAL;
  if ((a.runs == nullptr) != (a.run_ptr == nullptr)) return DTA_EINVAL;
  if (a.dkv_units && (a.n_units <= 0 || a.n_splits < 0 || (a.n_splits > 0 && (!a.dkv_splits || !a.dkv_ws)))) return DTA_EINVAL;
  if (bwd && (a.which & 7) == 0) return DTA_EINVAL;
  if ((a.head_dim != 128 && a.head_dim != 64) || a.Hq % a.Hkv != 0 || (a.dtype != DTA_BF16 && a.dtype != DTA_F16 && a.dtype != DTA_F32) ||
      a.accumulate < 0 || a.accumulate > 2) return DTA_EUNSUPPORTED;
  if (!aligned16(a.q) || !aligned16(a.k) || !aligned16(a.v) || !aligned16(a.o) || !aligned16(a.out) || !aligned16(a.dout) || !aligned16(a.dq) ||
      !aligned16(a.dk) || !aligned16(a.dv) ||
      (a.q_st | a.q_sh | a.kv_st | a.kv_sh | a.v_st | a.v_sh | a.o_st | a.o_sh | a.dq_st | a.dq_sh | a.dkv_st | a.dkv_sh) % 8 != 0) return DTA_EALIGN;
  if (a.dtype == DTA_F32) return DTA_OK;
  // the tile DMA addresses a 64-row tile as scalar base + 32-bit lane offset: the token strides of the tiles it stages (K and V in the
  // forward, Q and dO in the backward) must keep 64 rows inside 4 GiB
  const int64_t s0 = bwd ? a.q_st : a.kv_st, s1 = bwd ? a.o_st : a.v_st;
  if (s0 < 0 || s1 < 0 || s0 > (1 << 24) || s1 > (1 << 24)) return DTA_EUNSUPPORTED;
  return DTA_OK;
}

// Explicit instantiation in the order the kernels have always had in the device image (uncapped forms: forward then backward of each;
// capped forms: both forwards, then both backwards).  Without it their order follows the dispatch code above and moves with every edit of it.
template void launch_fwd<false, false>(const DtaAttnArgs&); template void launch_bwd<false, false>(const DtaAttnArgs&);
template void launch_fwd<true, false>(const DtaAttnArgs&); template void launch_bwd<true, false>(const DtaAttnArgs&);
template void launch_fwd<true, true>(const DtaAttnArgs&); template void launch_fwd<false, true>(const DtaAttnArgs&);
template void launch_bwd<true, true>(const DtaAttnArgs&); template void launch_bwd<false, true>(const DtaAttnArgs&);

int attn_call(const DtaAttnArgs& a, bool bwd) {
  if (const int e = check_args(a, bwd)) return e;
  DTA_REFUSE_IF_PRIOR_ERROR();
  if (a.dtype == DTA_F32)                                    // fp32 models: the plain-FMA correctness path (tree_attn_f32.hip)
    return bwd ? dta_attn_bwd_f32(a) : dta_attn_fwd_f32(a);
  dta_attn_form(a, [&](auto win, auto cap) {
    if (bwd) launch_bwd<decltype(win)::value, decltype(cap)::value>(a); else launch_fwd<decltype(win)::value, decltype(cap)::value>(a);
  });
  return DTA_LAUNCH_STATUS();
}

}  // namespace

extern "C" int dta_tree_attn_fwd(const void* q, const void* k, const void* v, void* out, float* lse,
                                 const int32_t* subtree_end, const int32_t* run_ptr, const int32_t* runs,
                                 int32_t Tq, int32_t Tk, int32_t q_offset, int32_t Hq, int32_t Hkv, int32_t head_dim,
                                 int64_t q_st, int64_t q_sh, int64_t kv_st, int64_t kv_sh, int64_t v_st, int64_t v_sh, int64_t o_st, int64_t o_sh,
                                 float scale, int32_t dtype, const int32_t* win_lo, int32_t window, float softcap, void* stream) {
  DtaAttnArgs a{};
  a.q = q; a.k = k; a.v = v; a.out = out; a.lse_w = lse; a.subtree_end = subtree_end; a.run_ptr = run_ptr; a.runs = runs;
  a.Tq = Tq; a.Tk = Tk; a.q_offset = q_offset; a.Hq = Hq; a.Hkv = Hkv; a.head_dim = head_dim;
  a.q_st = q_st; a.q_sh = q_sh; a.kv_st = kv_st; a.kv_sh = kv_sh; a.v_st = v_st; a.v_sh = v_sh; a.o_st = o_st; a.o_sh = o_sh;
  a.scale = scale; a.dtype = dtype; a.win_lo = win_lo; a.window = window; a.softcap = softcap; a.stream = static_cast<hipStream_t>(stream);
  return attn_call(a, false);
}

extern "C" int dta_tree_attn_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout,
                                 const float* lse, float* delta, void* dq, void* dk, void* dv,
                                 const int32_t* subtree_end, const int32_t* run_ptr, const int32_t* runs,
                                 const int32_t* ktile_qend,
                                 int32_t Tq, int32_t Tk, int32_t q_offset, int32_t Hq, int32_t Hkv, int32_t head_dim,
                                 int64_t q_st, int64_t q_sh, int64_t kv_st, int64_t kv_sh, int64_t v_st, int64_t v_sh, int64_t o_st, int64_t o_sh,
                                 int64_t dq_st, int64_t dq_sh, int64_t dkv_st, int64_t dkv_sh,
                                 float scale, int32_t dtype, int32_t accumulate, int32_t which,
                                 const int32_t* dkv_units, int32_t n_units, const int32_t* dkv_splits, int32_t n_splits, float* dkv_ws,
                                 const int32_t* win_lo, int32_t window, float softcap, void* stream) {
  DtaAttnArgs a{};
  a.q = q; a.k = k; a.v = v; a.o = out; a.dout = dout; a.lse_r = lse; a.delta = delta; a.dq = dq; a.dk = dk; a.dv = dv;
  a.subtree_end = subtree_end; a.run_ptr = run_ptr; a.runs = runs; a.ktile_qend = ktile_qend;
  a.dkv_units = dkv_units; a.n_units = n_units; a.dkv_splits = dkv_splits; a.n_splits = n_splits; a.dkv_ws = dkv_ws;
  a.Tq = Tq; a.Tk = Tk; a.q_offset = q_offset; a.Hq = Hq; a.Hkv = Hkv; a.head_dim = head_dim;
  a.q_st = q_st; a.q_sh = q_sh; a.kv_st = kv_st; a.kv_sh = kv_sh; a.v_st = v_st; a.v_sh = v_sh; a.o_st = o_st; a.o_sh = o_sh;
  a.dq_st = dq_st; a.dq_sh = dq_sh; a.dkv_st = dkv_st; a.dkv_sh = dkv_sh; a.scale = scale; a.dtype = dtype; a.accumulate = accumulate; a.which = which;
  a.win_lo = win_lo; a.window = window; a.softcap = softcap; a.stream = static_cast<hipStream_t>(stream);
  return attn_call(a, true);
}
