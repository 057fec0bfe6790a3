// MXFP8 workload kernels (gfx950 / CDNA4). Part of workload.hip: included
// inside its anonymous namespace after gemm_bf16_nt_8ph, whose tile map,
// half-tile row assignment (p8_src_row), LDS constants and packed epilogue
// (p8_store_c) are used here unchanged.
//
//   gemm_mxfp8_nt   C[M,N] = Σ_k (A[m,k]·2^(SA[m,k/32]−127)) · (B[n,k]·2^(SB[n,k/32]−127))
//                   A, B OCP e4m3 ("fn") row-major [rows, K]; SA, SB E8M0 bytes
//                   [rows, K/32]; fp32 accumulate on
//                   v_mfma_scale_f32_16x16x128_f8f6f4, bf16 out (RNE). The
//                   unscaled flavour loads no scales and passes 127 (2^0).
//   quantize_mxfp8  bf16 [R,K] → e4m3 [R,K] + E8M0 [R,K/32], OCP MX rule.
//
// gemm_mxfp8_nt design
//   Tile. 256×256×128, 512 threads, 8 waves as 2×4, 128×64 of C per wave, one
//   block per CU, two K-tiles in LDS (128 KiB). A 128-byte fp8 K-tile row has
//   the byte geometry of the bf16 kernel's 64-element row, so the staging is
//   that kernel's byte for byte: each wave writes LDS rows [16·wave, +16) of
//   the four 16 KiB half-tiles (A0 A1 B0 B1) with two global_load_lds_dwordx4
//   each, 16-byte chunk c of row r stored at chunk c ^ (r & 7) by swizzling
//   the per-lane SOURCE address. Per-lane offsets are 32-bit: the host
//   requires M·K and N·K < 2^32.
//   Fragments. The MFMA takes K as two halves of 64: lane l holds row l&15
//   and, with g = l>>4, k-bytes 16g .. 16g+15 in its first four operand
//   registers and 64+16g .. 64+16g+15 in the last four, the logical chunks g
//   and g+4 of its LDS row, fetched by two ds_read_b128 through the XOR. The
//   rule relied on, to be checked against the ISA document: the scale operand
//   of lane group g applies to k-bytes 32g .. 32g+31 of row l&15, and those
//   bytes live in lane groups 2(g&1) and 2(g&1)+1, in operand registers
//   4(g>>1) .. 4(g>>1)+3. So a lane passes the E8M0 byte of K-block g although
//   its own data belong to blocks g>>1 and 2 + (g>>1). The evidence is one
//   observation on the MI355X and the exact-integer test: feeding a lane 32
//   contiguous k-bytes (one whole MX block) gave a right unscaled product and
//   a wrong scaled one, its first half scaled by block g>>1 and its second by
//   2 + (g>>1).
//   Bank conflicts, by argument (no counter run was made for this kernel): the
//   two reads are chunk g and chunk g ^ 4 of rows ≡ l&15 (mod 16) through the
//   same XOR, exactly the ks = 0 and ks = 1 reads of gemm_bf16_nt_8ph, whose
//   ds_read_b128 measured conflict-free (profiles/r1_pmc_kernels.md).
//   Compute. By quadrants: a 64×32 quadrant of the wave's 128×64 is 4×2 MFMAs
//   of 16×16×128, operands entered as (B, A) so each lane ends with four
//   consecutive columns of a C row (what p8_store_c packs). Fragments of a
//   phase take 64 VGPRs (one A subtile 32, both B subtiles 32), accumulators
//   128.
//   Scales. Per K-tile a row has one dword of four scale bytes. A lane loads
//   the dword of each row it feeds (8 for A, 4 for B; they hit in L2) with
//   raw buffer loads issued together with the DMA of that K-tile, and
//   extracts its byte g into byte 0 after the wait (op_sel 0). Buffer loads
//   because they take a scalar offset: as plain global loads the twelve
//   addresses were kept as 64-bit VGPR pairs and the kernel spilled.
//   Pipeline. Two buffers. At the top of K-tile k all DMA and scale loads of
//   tile k+1 go to the other buffer (nothing on the last tile); tile k is
//   computed; then s_waitcnt vmcnt(0) and one barrier. The other buffer was
//   last read before the previous barrier. A final vmcnt(0) precedes the
//   epilogue so no LDS-DMA outlives the block.
//   Not done here: the counted-vmcnt, staggered-barrier 8-phase schedule of
//   gemm_bf16_nt_8ph is the natural follow-up. The scale loads change every
//   count in it, and a wrong count is a hang, so it wants its own change.

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <bool SCALED>
__global__ __launch_bounds__(P8_THREADS) void gemm_mxfp8_nt(const uint8_t* __restrict__ A,
                                                           const uint8_t* __restrict__ B,
                                                           const uint8_t* __restrict__ SA,
                                                           const uint8_t* __restrict__ SB,
                                                           uint16_t* __restrict__ C, int M, int N, int K) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];

  int m0, n0;
  p8_tile_origin(M, N, m0, n0);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave >> 2;  // 2 wave rows × 4 wave columns
  const int wc = wave & 3;
  const int nk = K / 128;

  // Staging, as in gemm_bf16_nt_8ph: lane l covers LDS row 16·wave + 8s + l/8,
  // physical chunk l%8, loaded from logical chunk (l%8) ^ (row & 7).
  uint32_t src_off[4][2];  // byte offset of this lane's 16 B at k = 0
#pragma unroll
  for (int kind = 0; kind < 4; ++kind)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int r = wave * 16 + s * 8 + (lane >> 3);
      const int chunk = (lane & 7) ^ (r & 7);
      const int grow = (kind < 2 ? m0 : n0) + p8_src_row(kind, r);
      src_off[kind][s] = static_cast<uint32_t>(grow) * static_cast<uint32_t>(K) + chunk * 16;
    }

  const int frow = lane & 15;
  const int g = lane >> 4;
  const int rd0 = (g ^ (frow & 7)) * 16;  // chunk g; chunk g + 4 is rd0 ^ 64
  const int a_row = wr * 64 + frow;                        // LDS row within an A half-tile
  const int b_row = wc * 32 + frow;                        // … within a B half-tile

  // Scale dwords of K-tile 0 for the rows this lane feeds: A row group i
  // (= mh·4 + mt) is tile row wr·128 + 16i + frow, B group j (= nh·2 + nt) is
  // tile row wc·64 + 16j + frow. K/32 is a multiple of 4: the dwords are aligned.
  // They are buffer loads: one VGPR (frow·K/32) addresses all twelve and the
  // rest of the offset is wave-uniform and scalar. The descriptor's range check
  // covers only the VGPR part; staying in bounds rests on the host's shape checks.
  const int kq = K / 32;
  __amdgpu_buffer_rsrc_t sa_rsrc, sb_rsrc;
  if constexpr (SCALED) {
    sa_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(SA), 0, M * kq, 0x00020000);
    sb_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(SB), 0, N * kq, 0x00020000);
  }
  const int s_lane = frow * kq;
  const int sa_wave = (m0 + wr * 128) * kq;
  const int sb_wave = (n0 + wc * 64) * kq;
  uint32_t sa_next[8], sb_next[4];  // dwords in flight
  int sa[8], sb[4];                 // this lane's byte of the current K-tile
#pragma unroll
  for (int i = 0; i < 8; ++i) sa[i] = 127;
#pragma unroll
  for (int j = 0; j < 4; ++j) sb[j] = 127;

  auto stage = [&](int buf, int kt) {
#pragma unroll
    for (int kind = 0; kind < 4; ++kind)
#pragma unroll
      for (int s = 0; s < 2; ++s)
        __builtin_amdgcn_global_load_lds(
            (__attribute__((address_space(1))) void*)((kind < 2 ? A : B) + (src_off[kind][s] + kt * 128u)),
            (__attribute__((address_space(3))) void*)(smem + buf * P8_BUF + kind * P8_HALF + (wave * 16 + s * 8) * 128),
            16, 0, 0);
    if constexpr (SCALED) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        sa_next[i] = __builtin_amdgcn_raw_buffer_load_b32(sa_rsrc, s_lane, sa_wave + i * 16 * kq + kt * 4, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        sb_next[j] = __builtin_amdgcn_raw_buffer_load_b32(sb_rsrc, s_lane, sb_wave + j * 16 * kq + kt * 4, 0);
    }
  };
  // After vmcnt(0): the staged tile becomes the current one.
  auto take_scales = [&]() {
    if constexpr (SCALED) {
#pragma unroll
      for (int i = 0; i < 8; ++i) sa[i] = __builtin_amdgcn_ubfe(sa_next[i], 8 * g, 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) sb[j] = __builtin_amdgcn_ubfe(sb_next[j], 8 * g, 8);
    }
  };

  i32x8 af[4];     // A fragments of one 64-row subtile
  i32x8 bq[2][2];  // B fragments of both 32-column subtiles
  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto fragment = [&](const unsigned char* row) {
    const i32x4 lo = *reinterpret_cast<const i32x4*>(row + rd0);
    const i32x4 hi = *reinterpret_cast<const i32x4*>(row + (rd0 ^ 64));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  };
  auto read_a = [&](int buf, int mh) {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) af[mt] = fragment(smem + buf * P8_BUF + mh * P8_HALF + (a_row + mt * 16) * 128);
  };
  auto read_b = [&](int buf, int nh) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
      bq[nh][nt] = fragment(smem + buf * P8_BUF + (2 + nh) * P8_HALF + (b_row + nt * 16) * 128);
  };
  // (B, A): the product is the 16×16 tile of Cᵀ, so a lane holds row m = l&15,
  // columns 4g..4g+3 of C. The first scale operand belongs to B, the second to A.
  auto mfma = [&](int mh, int nh) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
        acc[mh * 4 + mt][nh * 2 + nt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            bq[nh][nt], af[mt], acc[mh * 4 + mt][nh * 2 + nt], 0, 0, 0, sb[nh * 2 + nt], 0, sa[mh * 4 + mt]);
    __builtin_amdgcn_s_setprio(0);
  };

  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  take_scales();

  // One K-tile from buffer `buf`. sched_barrier(0) pins the order of the
  // steps: left alone the compiler hoists every fragment read above the first
  // MFMA, which costs 32 more VGPRs and spills.
  auto compute = [&](int buf) {
    __builtin_amdgcn_sched_barrier(0);
    read_b(buf, 0);
    read_b(buf, 1);
    read_a(buf, 0);
    mfma(0, 0);
    mfma(0, 1);
    __builtin_amdgcn_sched_barrier(0);
    read_a(buf, 1);
    mfma(1, 1);
    mfma(1, 0);
    __builtin_amdgcn_sched_barrier(0);
  };
  // The loop body has no branch (the last tile, which stages nothing, is
  // peeled): across one the compiler sinks the MFMAs below the barrier and
  // the DMA no longer overlaps them.
  for (int kt = 0; kt + 1 < nk; ++kt) {
    stage((kt & 1) ^ 1, kt + 1);  // in flight while this tile is consumed
    compute(kt & 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tile kt+1 and its scales have landed
    __builtin_amdgcn_s_barrier();                     // … for every wave, and all reads of this buffer retired
    take_scales();
  }
  compute((nk - 1) & 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no LDS-DMA may outlive the block

  p8_store_c(acc, C, N, m0, n0, wr, wc, lane);
}

// quantize_mxfp8: one pass, 16 bytes (8 bf16) per lane, four lanes per MX
// block of 32. Per block X = floor(log2(amax)) − 8 clamped to [−127, 127],
// scale byte X + 127, element RNE_e4m3(clamp(v·2^−X, ±448)); an all-zero
// block gets scale byte 127. In biased-exponent terms, with e the exponent
// field of amax as a float: scale byte = max(e − 8, 0) (e ≤ 254 keeps it
// ≤ 246, and subnormal amax, e = 0, lands on the clamp), and 2^−X is the
// float whose exponent field is 254 − scale byte (8..254: always normal), so
// the scaling is an exact multiply. |v|·2^−X < 2^9 is clamped to 448 in fp32
// before the conversion, which therefore never sees an overflow. amax is
// taken on the bit patterns (non-negative floats order as integers) with two
// quad_perm DPP steps; the four scale bytes of a 16-lane row are OR-ed
// together with two row rotations and stored as one dword by the row's first
// lane. Inputs are finite by contract.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
  return __builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, 0xf, 0xf, false);
}

// Compiled without packed fp32 arithmetic (v_pk_mul/add/fma_f32), so the eight
// scale-and-clamp multiplies stay single instructions whatever the vectoriser
// would make of them; per kernel, the rest of workload.hip is built as before.
__attribute__((target("no-packed-fp32-ops")))
__global__ __launch_bounds__(256) void quantize_mxfp8(const u32x4* __restrict__ x, u32x2* __restrict__ q,
                                                      uint8_t* __restrict__ scales, size_t n8) {
  // n8 (16-byte vectors) is a multiple of 4, so a block's four lanes are in or
  // out of range together; lanes past the end stay active for the DPP steps
  // and only skip the memory accesses.
  const size_t t = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  const bool live = t < n8;
  const u32x4 raw = live ? x[t] : u32x4{0, 0, 0, 0};
  float v[8];
  uint32_t amax = 0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const uint32_t lo = raw[p] << 16, hi = raw[p] & 0xffff0000u;  // bf16 → fp32 is a shift
    v[2 * p] = __builtin_bit_cast(float, lo);
    v[2 * p + 1] = __builtin_bit_cast(float, hi);
    amax = max(amax, max(lo & 0x7fffffffu, hi & 0x7fffffffu));
  }
  amax = max(amax, dpp<0xB1>(amax));  // quad_perm:[1,0,3,2]
  amax = max(amax, dpp<0x4E>(amax));  // quad_perm:[2,3,0,1]
  const uint32_t e = amax >> 23;
  const uint32_t sbyte = amax == 0 ? 127u : (e > 8 ? e - 8 : 0u);
  const float inv = __builtin_bit_cast(float, (254u - sbyte) << 23);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = __builtin_amdgcn_fmed3f(v[i] * inv, -448.f, 448.f);
  int w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], w0, true);
  int w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[4], v[5], 0, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[6], v[7], w1, true);
  if (live) q[t] = u32x2{static_cast<uint32_t>(w0), static_cast<uint32_t>(w1)};

  uint32_t word = sbyte << (8 * ((threadIdx.x >> 2) & 3));
  word |= dpp<0x124>(word);  // row_ror:4
  word |= dpp<0x128>(word);  // row_ror:8
  if ((threadIdx.x & 15) == 0 && live) {
    if (t + 16 <= n8) {
      *reinterpret_cast<uint32_t*>(scales + (t >> 2)) = word;
    } else {  // last, partial group of blocks: byte stores
      for (size_t j = 0; t + 4 * j < n8; ++j) scales[(t >> 2) + j] = static_cast<uint8_t>(word >> (8 * j));
    }
  }
}

bool g_mxfp8_attr[2] = {false, false};

template <bool SCALED>
const char* launch_mxfp8_kernel(const void* a, const void* b, const void* sa, const void* sb, void* c, int m, int n,
                                int k, hipStream_t stream) {
  auto kernel = gemm_mxfp8_nt<SCALED>;
  if (!g_mxfp8_attr[SCALED]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            P8_LDS) != hipSuccess)
      return "gemm_mxfp8_nt: cannot reserve LDS";
    g_mxfp8_attr[SCALED] = true;
  }
  hipLaunchKernelGGL(kernel, dim3((m / 256) * (n / 256)), dim3(P8_THREADS), P8_LDS, stream,
                     static_cast<const uint8_t*>(a), static_cast<const uint8_t*>(b), static_cast<const uint8_t*>(sa),
                     static_cast<const uint8_t*>(sb), static_cast<uint16_t*>(c), m, n, k);
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? nullptr : hipGetErrorString(err);
}

// sa == sb == nullptr selects the unscaled flavour. No smaller-tile fallback.
const char* launch_gemm_mxfp8(const void* a, const void* b, const void* sa, const void* sb, void* c, int m, int n,
                              int k, hipStream_t stream) {
  if (m <= 0 || n <= 0 || k <= 0 || m % 256 || n % 256 || k % 128 ||
      static_cast<uint64_t>(m) * k >= (1ull << 32) || static_cast<uint64_t>(n) * k >= (1ull << 32))
    return "gemm_mxfp8_nt: needs M,N multiples of 256, K of 128, M*K and N*K < 2^32";
  if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15)
    return "gemm_mxfp8_nt: A, B and C must be 16-byte aligned";
  if ((sa == nullptr) != (sb == nullptr)) return "gemm_mxfp8_nt: give both scale tensors or neither";
  if ((reinterpret_cast<uintptr_t>(sa) | reinterpret_cast<uintptr_t>(sb)) & 3)
    return "gemm_mxfp8_nt: scales must be 4-byte aligned";
  return sa ? launch_mxfp8_kernel<true>(a, b, sa, sb, c, m, n, k, stream)
            : launch_mxfp8_kernel<false>(a, b, sa, sb, c, m, n, k, stream);
}

const char* launch_quantize_mxfp8(const void* x, void* q, void* scales, long long rows, long long k,
                                  hipStream_t stream) {
  if (rows <= 0 || k <= 0 || k % 32) return "quantize_mxfp8: needs rows > 0 and K a positive multiple of 32";
  if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(q) & 7) ||
      (reinterpret_cast<uintptr_t>(scales) & 3))
    return "quantize_mxfp8: x must be 16-byte, q 8-byte and scales 4-byte aligned";
  if (rows > (1ll << 40) / k) return "quantize_mxfp8: tensor too large for one pass";
  const size_t n8 = static_cast<size_t>(rows) * static_cast<size_t>(k) / 8;
  hipLaunchKernelGGL(quantize_mxfp8, dim3(static_cast<unsigned>((n8 + 255) / 256)), dim3(256), 0, stream,
                     static_cast<const u32x4*>(x), static_cast<u32x2*>(q), static_cast<uint8_t*>(scales), n8);
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? nullptr : hipGetErrorString(err);
}
