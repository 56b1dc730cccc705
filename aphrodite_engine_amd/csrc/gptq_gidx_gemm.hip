// W4A16 decode GEMM on CHECKPOINT-ORDER GPTQ weights with a per-row group map (g_idx) for gfx950.
//
// Stands in for the reference's gemm_half_q_half_alt_4bit_kernel (kernels/quantization/gptq/q_gemm.cu:1184-1281), the
// kernel it runs for act-order (desc_act) checkpoints under row-parallel tensor parallelism: those layers keep their
// rows in checkpoint order (gptq.py:137-139, ExllamaState.UNUSED), every row k finds its scale / zero point through
// g_idx[k], and the group count G is that of the UNSHARDED matrix (no relation between K and G).  Before this file the
// form was reconstructed to a [K, N] 16-bit matrix and multiplied by a library GEMM at every batch size.
//
// Design (DESIGN.md "gptq_gidx_gemm"):
//   * Work split: grid = (N / 64 column tiles) x (K slices).  A workgroup is 8 waves that share ONE column tile and
//     take the 32-k steps of the slice round-robin; they reduce through LDS in a fixed order.  K slices across
//     workgroups go through an fp32 workspace (write-through stores) and a per-tile ticket: the last arriver adds the
//     slices IN SLICE ORDER (bits independent of arrival order), stores the output and resets the ticket, so the
//     call replays under a HIP graph.  The tickets are a zero-initialised __device__ array of this module: nothing is
//     allocated on the launch path.  (Calls of one process are stream-ordered, as for aphro_wna16_gemm_rowmajor: two
//     of them running CONCURRENTLY on one device would share tickets.)
//   * Weights: one checkpoint word is 8 consecutive k of one column = a B fragment of v_mfma_f32_16x16x32_f16 for
//     lane (g = lane >> 4, c = lane & 15), k = 8g..8g+7.  A dwordx4 load gives the lane columns n0 + 4c .. + 3 (four
//     MFMA n-tiles); 16 lanes read 256 contiguous bytes; every word is read from HBM once, nontemporal, two 512-k
//     chunks ahead of its use.
//   * The mask 0x000f000f pulls the nibble pair (k0, k4) out of a checkpoint word, then (k1, k5), (k2, k6), (k3, k7):
//     the B fragment's register order is k = 0,4,1,5,2,6,3,7.  The SAME order is put into the A fragments when the
//     workgroup stages its activations (once per 512-k chunk, fragment-major in LDS: one conflict-free ds_read_b128 per
//     fragment); no VALU is spent on re-ordering B.
//   * Scale and zero point differ per ROW, so the weights are dequantised completely in registers: the workgroup stages
//     the scale / zero columns of its tile for all G groups into LDS once, as one 32-bit entry per (group, column) =
//     half2(1024 + z + zero_offset, scale); the g_idx values of a chunk are read once, clamped to [0, G - 1] (a bad
//     entry gives wrong numbers, never an out-of-range read) and kept as 16-bit table rows.  A lane fetches the entries
//     of its 8 rows x 4 columns with 8 ds_read_b128 per k-step; v_perm_b32 pairs them like the nibbles.
//   * f16: (1024 + q) - (1024 + z) is exact, one multiply by the scale = ONE rounding of the exact product: the bits
//     of the reconstruct kernel's weight (q_gemm.cu:1427-1431, aphro_gptq_dequant).  fp32 accumulation in the MFMA.
//   * bf16: the activations go through the project's saturating bf16 -> f16 conversion (load_a_frag<BFloat>'s rule,
//     common.h) and the scales are converted to f16 when the table is built (exact for every bf16 scale >= 2^-14, i.e.
//     every real checkpoint: a bf16 significand fits an f16 one).  Chosen over the bf16 MFMA on weights rounded to bf16
//     because the f16 weight keeps 11 significand bits of (q - z) * s where bf16 keeps 8, and because one dequant code
//     path serves both types.  Accumulation is fp32, the output is rounded once to bf16.
#include "common.h"

namespace aphro {

constexpr int GX_NWV = 8;                       // waves per workgroup
constexpr int GX_NT = GX_NWV * 64;
constexpr int GX_CHUNK = 16;                    // 32-k steps per staged activation chunk (512 k)
constexpr int GX_SPW = GX_CHUNK / GX_NWV;       // k-steps per wave per chunk
constexpr int GX_ROWP = 68;                     // floats per row of a reduce slot (64 + 4: the four row groups of a store
                                                // land 64 bytes apart in the banks)
constexpr int GX_MAX_TILES = 4096;              // tickets
constexpr int GX_LDS_MAX = 160 * 1024;

// bytes of the region that holds the staged activation chunk during the K loop (16 KiB per m-tile) and the four reduce
// slots after it (17 KiB per m-tile)
constexpr int gx_region_bytes(int mt) { return (GX_NWV / 2) * 16 * mt * GX_ROWP * 4; }
constexpr int gx_lds_bytes(int groups, int mt) { return groups * 256 + gx_region_bytes(mt) + GX_CHUNK * 32 * 2 + 16; }

__device__ unsigned g_gidx_tickets[GX_MAX_TILES];   // one per column tile; zero between launches

struct GidxParams {
  const uint16_t* a;       // [M, lda]
  const uint32_t* qw;      // [K/8, N] checkpoint order
  const uint32_t* qz;      // [G, N/8]
  const uint16_t* sc;      // [G, N]
  const int32_t* g_idx;    // [K]
  uint16_t* c;             // [M, N]
  float* partial;          // [ksplit, M, N] (ksplit > 1)
  int M, N, K, G, lda, zero_offset;
  int steps_per_slice;     // 32-k steps per blockIdx.y
  int ksplit;
};

__device__ __forceinline__ void gx_st_wt(float* p, f32x4 v) {   // write-through: visible to the other XCDs' loads below
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void gx_ld_coh8(f32x4 (&v)[8], const float* const (&p)[8]) {
  asm volatile(
      "global_load_dwordx4 %0, %8, off sc0 sc1\n\tglobal_load_dwordx4 %1, %9, off sc0 sc1\n\t"
      "global_load_dwordx4 %2, %10, off sc0 sc1\n\tglobal_load_dwordx4 %3, %11, off sc0 sc1\n\t"
      "global_load_dwordx4 %4, %12, off sc0 sc1\n\tglobal_load_dwordx4 %5, %13, off sc0 sc1\n\t"
      "global_load_dwordx4 %6, %14, off sc0 sc1\n\tglobal_load_dwordx4 %7, %15, off sc0 sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7])
      : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5]), "v"(p[6]), "v"(p[7])
      : "memory");
}

// One checkpoint word (column t of the lane) -> the scaled f16 B fragment in register order k = 0,4,1,5,2,6,3,7.
// e[kk][t] = table entry of row kk: low half 1024 + z, high half the scale.
__device__ __forceinline__ f16x8 gx_dequant(uint32_t w, const u32x4 (&e)[8], int t) {
  u32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t q = ((w >> (4 * j)) & 0x000f000fu) | 0x64006400u;                  // half2(1024 + q[j], 1024 + q[j + 4])
    const uint32_t zp = __builtin_amdgcn_perm(e[j + 4][t], e[j][t], 0x05040100u);     // half2(1024 + z[j], 1024 + z[j + 4])
    const uint32_t sp = __builtin_amdgcn_perm(e[j + 4][t], e[j][t], 0x07060302u);     // half2(s[j], s[j + 4])
    const f16x2 d = (__builtin_bit_cast(f16x2, q) - __builtin_bit_cast(f16x2, zp)) * __builtin_bit_cast(f16x2, sp);
    r[j] = __builtin_bit_cast(uint32_t, d);
  }
  return __builtin_bit_cast(f16x8, r);
}

template <typename T, int MT>
__global__ __launch_bounds__(GX_NT) void gptq_gidx_gemm_kernel(GidxParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gx_lds[];
  uint32_t* table = reinterpret_cast<uint32_t*>(gx_lds);                              // [G][64]
  unsigned char* region = gx_lds + (size_t)p.G * 256;                                 // A chunk, later the reduce slots
  uint16_t* grow = reinterpret_cast<uint16_t*>(region + gx_region_bytes(MT));         // [512] clamped group of each chunk row
  int* flag = reinterpret_cast<int*>(region + gx_region_bytes(MT) + GX_CHUNK * 32 * 2);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int tile = blockIdx.x, ky = blockIdx.y;
  const int n0 = tile * 64;
  const int s_begin = ky * p.steps_per_slice;                                         // host: s_begin < K / 32 for every slice
  const int s_end = min(p.K >> 5, s_begin + p.steps_per_slice);
  const int nchunks = (s_end - s_begin + GX_CHUNK - 1) / GX_CHUNK;

  // ---- loads; every address is clamped into the slice, so no load is conditional --------------------------------
  auto load_w = [&](u32x4 (&wd)[GX_SPW], int ch) {
#pragma unroll
    for (int q = 0; q < GX_SPW; ++q) {
      const int s = min(s_begin + ch * GX_CHUNK + wave + GX_NWV * q, s_end - 1);
      wd[q] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p.qw + (size_t)(4 * s + g) * p.N + n0 + 4 * c));
    }
  };
  u16x8 areg[2 * MT];
  int greg;
  auto load_a = [&](int ch) {          // unit u = (k-step ks, m-tile i, lane (g, m)): the 8 k of one A fragment lane
#pragma unroll
    for (int j = 0; j < 2 * MT; ++j) {
      const int u = tid + j * GX_NT, l = u & 63, rest = u >> 6;
      const int i = rest % MT, ks = rest / MT;
      const int row = min(16 * i + (l & 15), p.M - 1);          // rows >= M read row M - 1; never stored
      const int s = min(s_begin + ch * GX_CHUNK + ks, s_end - 1);
      areg[j] = *reinterpret_cast<const u16x8*>(p.a + (size_t)row * p.lda + 32 * s + 8 * (l >> 4));
    }
    greg = p.g_idx[min((s_begin + ch * GX_CHUNK) * 32 + tid, p.K - 1)];
  };
  auto store_a = [&]() {
#pragma unroll
    for (int j = 0; j < 2 * MT; ++j) {
      u16x8 v = areg[j];
      if constexpr (!__is_same(T, Half)) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = bf16_bits_to_f16_bits_sat(v[e]);
      }
      const u16x8 o = {v[0], v[4], v[1], v[5], v[2], v[6], v[3], v[7]};               // the B fragment's nibble order
      *reinterpret_cast<u16x8*>(region + (size_t)(tid + j * GX_NT) * 16) = o;
    }
    grow[tid] = (uint16_t)min(max(greg, 0), p.G - 1);
  };

  u32x4 w0[GX_SPW], w1[GX_SPW], w2[GX_SPW];
  load_w(w0, 0);
  load_w(w1, 1);
  load_a(0);

  // ---- the tile's scale / zero columns of every group, in the form the dequant consumes --------------------------
  // unit = (group, 8 columns): one zero-point word + 16 bytes of scales -> 8 entries; 4 units' loads in flight per thread
  const int units = p.G * 8;
  for (int base = 0; base < units; base += 4 * GX_NT) {
    uint32_t zw[4];
    u16x8 s8[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int u = min(base + j * GX_NT + tid, units - 1), grp = u >> 3, cb = u & 7;
      zw[j] = p.qz[(size_t)grp * (p.N >> 3) + (n0 >> 3) + cb];
      s8[j] = *reinterpret_cast<const u16x8*>(p.sc + (size_t)grp * p.N + n0 + 8 * cb);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int u = base + j * GX_NT + tid;
      if (u < units) {
        uint32_t e[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          uint32_t s = s8[j][i];
          if constexpr (!__is_same(T, Half)) s = bf16_bits_to_f16_bits_sat((uint16_t)s);
          e[i] = (0x6400u + ((((zw[j] >> (4 * i)) & 0xfu) + (uint32_t)p.zero_offset) & 0x3ffu)) | (s << 16);
        }
        *reinterpret_cast<u32x4*>(table + u * 8) = u32x4{e[0], e[1], e[2], e[3]};
        *reinterpret_cast<u32x4*>(table + u * 8 + 4) = u32x4{e[4], e[5], e[6], e[7]};
      }
    }
  }
  store_a();
  __syncthreads();

  f32x4 acc[MT][4];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int ch = 0; ch < nchunks; ++ch) {
    load_a(ch + 1);                    // (past the last chunk: clamped re-reads, never used)
    load_w(w2, ch + 2);
#pragma unroll
    for (int q = 0; q < GX_SPW; ++q) {
      const int ks = wave + GX_NWV * q;
      if (s_begin + ch * GX_CHUNK + ks < s_end) {
        const u16x8 gi = *reinterpret_cast<const u16x8*>(grow + ks * 32 + 8 * g);
        u32x4 e[8];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) e[kk] = *reinterpret_cast<const u32x4*>(table + (int)gi[kk] * 64 + 4 * c);
        f16x8 af[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) af[i] = *reinterpret_cast<const f16x8*>(region + (size_t)((ks * MT + i) * 64 + lane) * 16);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const f16x8 b = gx_dequant(w0[q][t], e, t);
#pragma unroll
          for (int i = 0; i < MT; ++i) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], b, acc[i][t], 0, 0, 0);
        }
      }
    }
    __syncthreads();                   // every wave is past its reads of chunk ch
    store_a();
    __syncthreads();
#pragma unroll
    for (int q = 0; q < GX_SPW; ++q) { w0[q] = w1[q]; w1[q] = w2[q]; }
  }
  // (the last store_a + barrier: the region is free)

  // ---- 8 waves -> 1 through LDS, fixed order: slot w = wave w + wave w + 4, then slots 0..3 in order ----------------
  float* slots = reinterpret_cast<float*>(region);                                    // [4][16 MT][GX_ROWP]
  auto slot_at = [&](int sl, int i, int r) { return slots + ((size_t)(sl * 16 * MT + 16 * i + 4 * g + r)) * GX_ROWP + 4 * c; };
  if (wave >= GX_NWV / 2) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        *reinterpret_cast<f32x4*>(slot_at(wave - GX_NWV / 2, i, r)) = f32x4{acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]};
  }
  __syncthreads();
  if (wave < GX_NWV / 2) {             // (a lane rewrites exactly the 16-byte pieces it read)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        f32x4* sp = reinterpret_cast<f32x4*>(slot_at(wave, i, r));
        *sp = f32x4{acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]} + *sp;
      }
  }
  __syncthreads();
  constexpr int UNITS = 16 * MT * 16;  // (row, 4 columns)
  const bool mine = tid < UNITS;
  const int row = min(tid >> 4, 16 * MT - 1), c4 = tid & 15;
  f32x4 sum = *reinterpret_cast<const f32x4*>(slots + (size_t)row * GX_ROWP + 4 * c4);
#pragma unroll
  for (int sl = 1; sl < GX_NWV / 2; ++sl) sum += *reinterpret_cast<const f32x4*>(slots + (size_t)(sl * 16 * MT + row) * GX_ROWP + 4 * c4);
  const bool live = mine && row < p.M;
  const int srow = min(row, p.M - 1);
  uint16_t* cp = p.c + (size_t)srow * p.N + n0 + 4 * c4;
  if (p.ksplit == 1) {
    if (live) *reinterpret_cast<u16x4*>(cp) = u16x4{T::from_f32(sum[0]), T::from_f32(sum[1]), T::from_f32(sum[2]), T::from_f32(sum[3])};
    return;
  }
  // ---- K slices: write-through partial, ticket, the last arriver adds the slices in slice order ---------------------
  if (live) gx_st_wt(p.partial + ((size_t)ky * p.M + srow) * p.N + n0 + 4 * c4, sum);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const unsigned old = __hip_atomic_fetch_add(g_gidx_tickets + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *flag = old == (unsigned)p.ksplit - 1u;
  }
  __syncthreads();
  if (*flag == 0) return;
  if (tid == 0) __hip_atomic_store(g_gidx_tickets + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const float* ptr[8];
  f32x4 v[8];
#pragma unroll
  for (int z = 0; z < 8; ++z) ptr[z] = p.partial + ((size_t)(z < p.ksplit ? z : 0) * p.M + srow) * p.N + n0 + 4 * c4;
  gx_ld_coh8(v, ptr);
  sum = v[0];
#pragma unroll
  for (int z = 1; z < 8; ++z)
    if (z < p.ksplit) sum += v[z];
  if (live) *reinterpret_cast<u16x4*>(cp) = u16x4{T::from_f32(sum[0]), T::from_f32(sum[1]), T::from_f32(sum[2]), T::from_f32(sum[3])};
}

// K slices: about one workgroup per CU, at most 8 slices, at least 8 k-steps (one per wave) in a slice -- every slice
// builds the whole scale / zero table of its tile, so thin slices pay for it again and again.
static void gidx_plan(int64_t N, int64_t K, int* steps_per_slice, int* ksplit) {
  const int64_t tiles = N / 64, total = K / 32;
  int64_t want = (device_cu_count() + tiles / 2) / tiles;
  want = want < 1 ? 1 : (want > 8 ? 8 : want);
  const int64_t by_len = total / GX_NWV < 1 ? 1 : total / GX_NWV;
  if (want > by_len) want = by_len;
  const int64_t per = (total + want - 1) / want;
  *steps_per_slice = (int)per;
  *ksplit = (int)((total + per - 1) / per);
}

template <typename T, int MT>
static int launch_gidx(const GidxParams& p, hipStream_t st) {
  const size_t lds = (size_t)gx_lds_bytes(p.G, MT);
  static bool attr_set_dev[APHRO_MAX_DEVICES] = {}; bool& attr_set = attr_set_dev[device_slot()];   // (one per instantiation)
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)gptq_gidx_gemm_kernel<T, MT>, hipFuncAttributeMaxDynamicSharedMemorySize, GX_LDS_MAX) != hipSuccess) {
      set_error("gptq_gemm_gidx: cannot raise the dynamic LDS limit");
      return APHRO_ERR_LAUNCH;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL((gptq_gidx_gemm_kernel<T, MT>), dim3((unsigned)(p.N / 64), (unsigned)p.ksplit), dim3(GX_NT), lds, st, p);
  APHRO_LAUNCH_CHECK();
  return APHRO_OK;
}

}  // namespace aphro

using namespace aphro;

extern "C" int aphro_gptq_gemm_gidx_supported(int64_t M, int64_t N, int64_t K, int64_t groups, int dtype) {
  if (dtype != APHRO_F16 && dtype != APHRO_BF16) return 0;
  if (M < 1 || M > 32 || N < 64 || N % 64 != 0 || N / 64 > GX_MAX_TILES || K < 32 || K % 32 != 0) return 0;
  if (groups < 1 || groups > 65535 || gx_lds_bytes((int)groups, 2) > GX_LDS_MAX) return 0;
  return K <= ((int64_t)1 << 26);     // (row and k indices are 32-bit in the kernel)
}

extern "C" size_t aphro_gptq_gemm_gidx_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  (void)K;
  const int64_t m = M < 32 ? M : 32;
  return (size_t)8 * (size_t)(m < 0 ? 0 : m) * (size_t)N * sizeof(float);   // up to 8 K slices of fp32 partials
}

extern "C" int aphro_gptq_gemm_gidx(const void* a, int64_t lda, const uint32_t* q_weight, const uint32_t* qzeros,
                                    const void* scales, const int32_t* g_idx, void* c, void* workspace,
                                    size_t workspace_bytes, int64_t M, int64_t N, int64_t K, int64_t groups,
                                    int zero_offset, int dtype, void* stream) {
  if (M == 0) return APHRO_OK;
  APHRO_CHECK(aphro_gptq_gemm_gidx_supported(M, N, K, groups, dtype), "gptq_gemm_gidx: M=%ld N=%ld K=%ld groups=%ld dtype=%d is not served",
              (long)M, (long)N, (long)K, (long)groups, dtype);
  APHRO_CHECK(a && q_weight && qzeros && scales && g_idx && c, "gptq_gemm_gidx: null tensor");
  APHRO_CHECK(((uintptr_t)a % 16) == 0 && lda % 8 == 0 && lda >= K && ((uintptr_t)q_weight % 16) == 0 &&
              ((uintptr_t)scales % 16) == 0 && ((uintptr_t)c % 8) == 0,
              "gptq_gemm_gidx: a, q_weight and scales must be 16-byte aligned (lda %% 8 == 0, lda >= K), c 8-byte aligned");
  APHRO_CHECK(zero_offset == 0 || zero_offset == 1, "gptq_gemm_gidx: zero_offset must be 0 or 1");
  GidxParams p;
  p.a = (const uint16_t*)a; p.qw = q_weight; p.qz = qzeros; p.sc = (const uint16_t*)scales; p.g_idx = g_idx;
  p.c = (uint16_t*)c; p.partial = nullptr;
  p.M = (int)M; p.N = (int)N; p.K = (int)K; p.G = (int)groups; p.lda = (int)lda; p.zero_offset = zero_offset;
  gidx_plan(N, K, &p.steps_per_slice, &p.ksplit);
  if (p.ksplit > 1) {
    const size_t need = (size_t)p.ksplit * M * N * sizeof(float);
    if (workspace == nullptr || workspace_bytes < need || ((uintptr_t)workspace % 16) != 0) {
      set_error("gptq_gemm_gidx: workspace %zu < %zu bytes", workspace_bytes, need);
      return APHRO_ERR_WORKSPACE;
    }
    p.partial = (float*)workspace;
  }
  hipStream_t st = (hipStream_t)stream;
  if (dtype == APHRO_F16) return M > 16 ? launch_gidx<Half, 2>(p, st) : launch_gidx<Half, 1>(p, st);
  return M > 16 ? launch_gidx<BFloat, 2>(p, st) : launch_gidx<BFloat, 1>(p, st);
}
