// MXFP4 decode GEMM (gfx950 / CDNA4). Part of workload.hip: included inside
// its anonymous namespace after gemm_mxfp4.h, whose operand formats, fragment
// map, scale selection (v_perm_b32 + op_sel) and p4_operand are used here
// unchanged. Launcher, checks and the Python binding are at the bottom.
//
//   gemm_mxfp4_skinny    C[M,N] = Σ_k (A[m,k]·2^(SA−127)) · (B[n,k]·2^(SB−127)),
//                        the product of gemm_mxfp4_nt for 1 ≤ M ≤ 64 (any M),
//                        N a multiple of 128, K of 256, K split over split_k
//                        blocks. split_k = 1: bf16 out (RNE). split_k > 1:
//                        fp32 partial tiles to workspace[s][m][n].
//   mxfp4_skinny_reduce  adds the split_k partials in ascending s, rounds once
//                        to bf16. No atomics anywhere: bit-identical reruns.
//
// Why another kernel. Decode is a batch of 1-64 rows against the whole weight
// matrix: every byte of B is used once, by one wave, and the time is B's
// bytes over HBM bandwidth. The 256² kernel runs N/256 blocks there and moves
// B through LDS; this one keeps every CU pulling on HBM and moves B straight
// into MFMA fragments.
//
// Work split. Grid (N/128, split_k), 256 threads. Block (x, s) owns columns
// 128x .. +127 and the contiguous K-slice of K/split_k elements starting at
// s·K/split_k, walked in 256-element K-steps (one 128-byte packed row, two
// MFMAs). Wave w owns B rows n0+32w .. +31 as two 16-row groups (nt) and all
// MT = ⌈M/16⌉ M-tiles: MT×2 accumulator tiles, 32 VGPRs at most. The kernel
// is a template on MT, so M ≤ 16 issues a quarter of the MFMAs, LDS reads and
// A staging of M = 64.
//
// B, the weights: global → VGPR in fragment layout, no LDS. Lane l (i = l&15,
// g = l>>4) loads the 16 bytes at 128·kt + 64·ks + 16·g of row n0+32w+16nt+i:
// MX block g (ks = 0) or 4+g (ks = 1) of that row, exactly what the MFMA
// wants from it. The two ks loads of a step cover whole 128-byte lines. The
// row's 8 scale bytes of the step come from one 8-byte load, and the
// v_perm_b32 of gemm_mxfp4_nt leaves byte g in byte 0 and byte 4+g in byte 1
// (op_sel 0 / 1). A step is 4 dwordx4 + 2 dwordx2 loads per wave, 20 VGPRs.
// SK_DEPTH steps are kept in flight per wave in a register ring whose slot
// is the step index mod SK_DEPTH, static because the step loop is unrolled
// over the A chunk. All of it is plain C++ loads: the compiler counts vmcnt
// per register and never drains the ring (checked in the assembly:
// vmcnt(6·(SK_DEPTH−1)) before a step's MFMAs). The loads are plain:
// non-temporal ones (SK_NT=1), meant to keep the once-used stream from
// pushing A and the workspace out of L2, measured 9-17 % slower. Past the end of the slice the ring loads B's and SB's first 16 / 8 bytes
// instead (all lanes one address, one L2 hit), so every step issues the same
// count and there is no branch around a load; the data is never used.
// Offsets are 32-bit per lane: the host requires N·K/2 < 2^32.
//
// A, the activations: through LDS, shared by the four waves. A chunk is
// SK_CHUNK K-steps × 16·MT rows × 128 bytes (64 KiB at MT = 4), staged by
// global_load_lds_dwordx4 with the XOR chunk swizzle on the SOURCE address
// (16-byte chunk c of row r at chunk c ^ (r & 7)), image [step][row][128].
// SA follows it as [step][row][8], staged by 4-byte global_load_lds. Rows at
// or above M read row M−1 (clamped source), so every load is in bounds; those
// rows are computed and never stored. Steps past the slice are not staged.
// One buffer, two barriers per chunk: stage, vmcnt(0), barrier, up to
// SK_CHUNK steps without any barrier, barrier. The vmcnt(0) also lands the B
// ring, which was issued before the DMA (loads return in order), so the ring
// is full when the steps start; where the grid has more blocks than CUs, two
// per CU (68 KiB LDS each at MT = 4, 2 waves per SIMD) cover each other's
// staging. Fragment reads are the
// ds_read_b128 pair of gemm_mxfp4_nt (rd0, rd0 ^ 64) and one ds_read_b64 for
// the row's 8 scale bytes, 16 rows × 8 bytes per lane group: conflict-free.
//
// MFMA. v_mfma_scale_f32_16x16x128_f8f6f4 cbsz:4 blgp:4, operands entered as
// (B, A): lane l ends with row m = 16mt + i, columns 16nt + 4g .. +3 of the
// wave's 16×32 strip, one 8-byte bf16 or one 16-byte fp32 store.
//
// Measured on the MI355X (profiles/mxfp4_skinny_ab.md), TB/s over B, SB, A,
// SA and C with the weights rotated through 512 MiB, stream_triad 5.72 in the
// same process: 28672×8192 weights 3.65 / 3.63 / 3.33 at M = 1 / 16 / 64,
// 8192×8192 2.79 / 2.71 / 2.35; the 256-row padded gemm_mxfp4_nt 1.88-1.94
// and 0.59-0.61. Depth 1, 2, 4 lie within 3 % of each other and 8 (one wave
// per SIMD at MT = 4) is 5-10 % slower, SK_CHUNK 4 equals 8: the kernel is
// not bound by bytes in flight. What does bound it at 50-64 % of the triad
// was not found: no counter run was made. A quarter-wave of a fragment load
// gathers 16 bytes from each of 16 rows, the MFMA's layout, which costs four
// cache lookups per 64 bytes fetched; that is the first thing to count.

#ifndef SK_DEPTH
#define SK_DEPTH 2  // K-steps of B in flight per wave; divides SK_CHUNK
#endif
#ifndef SK_NT
#define SK_NT 0  // 1: non-temporal B and SB loads (measured 9-17 % slower)
#endif
#ifndef SK_CHUNK
#define SK_CHUNK 8  // K-steps of A per LDS chunk; even
#endif
static_assert(SK_CHUNK % SK_DEPTH == 0 && SK_CHUNK % 2 == 0, "ring slot must be static");
constexpr int SK_THREADS = 256;
constexpr int sk_lds(int mt) { return SK_CHUNK * 16 * mt * (128 + 8); }

typedef unsigned int u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));  // scale rows are 4-byte aligned
#if SK_NT
#define SK_STREAM_LOAD(p) __builtin_nontemporal_load(p)
#else
#define SK_STREAM_LOAD(p) (*(p))
#endif

template <int MT>
__global__ __launch_bounds__(SK_THREADS) void gemm_mxfp4_skinny(const uint8_t* __restrict__ A,
                                                               const uint8_t* __restrict__ B,
                                                               const uint8_t* __restrict__ SA,
                                                               const uint8_t* __restrict__ SB,
                                                               uint16_t* __restrict__ C, float* __restrict__ W, int M,
                                                               int N, int K, int nsteps) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  constexpr int ROWS = 16 * MT;
  constexpr int A_BYTES = SK_CHUNK * ROWS * 128;  // the scales follow the operand image

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15;
  const int g = lane >> 4;
  const uint32_t kb = K / 2;   // bytes per operand row
  const uint32_t kq = K / 32;  // scale bytes per row
  const int n0 = blockIdx.x * 128;
  const uint32_t kt0 = blockIdx.y * static_cast<uint32_t>(nsteps);  // first K-step of this block's slice

  // B ring. Offsets of this lane's bytes at the slice's first step.
  uint32_t b_off[2], sb_off[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const uint32_t row = n0 + 32 * wave + 16 * nt + i;
    b_off[nt] = row * kb + kt0 * 128u + 16 * g;
    sb_off[nt] = row * kq + kt0 * 8u;
  }
  i32x4 bq[SK_DEPTH][4];     // [slot][nt*2 + ks]
  u32x2 sb_raw[SK_DEPTH][2];  // [slot][nt]
#define SK_LOAD_B(slot, step)                                                                              \
  {                                                                                                        \
    const bool live_ = (step) < nsteps;                                                                    \
    _Pragma("unroll") for (int nt = 0; nt < 2; ++nt) {                                                     \
      const uint32_t o_ = live_ ? b_off[nt] + (step) * 128u : 0u;                                          \
      const uint32_t so_ = live_ ? sb_off[nt] + (step) * 8u : 0u;                                          \
      bq[slot][nt * 2 + 0] = SK_STREAM_LOAD(reinterpret_cast<const i32x4*>(B + o_));                       \
      bq[slot][nt * 2 + 1] = SK_STREAM_LOAD(reinterpret_cast<const i32x4*>(B + o_ + 64));                  \
      sb_raw[slot][nt] = SK_STREAM_LOAD(reinterpret_cast<const u32x2_a4*>(SB + so_));                      \
    }                                                                                                      \
  }

  // A staging. DMA q writes LDS bytes [1024q, +1024): flat rows 8q .. 8q+7 of
  // [step][row]; lane l covers flat row 8q + l/8, physical chunk l%8, loaded
  // from logical chunk (l%8) ^ (row & 7). Scale DMA q writes 64 dwords of
  // [step][row][2]: dword 64q + l.
#define SK_DMA(src, dst, bytes)                                                                            \
  __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)(src),                        \
                                   (__attribute__((address_space(3))) void*)(dst), bytes, 0, 0);
  constexpr int A_DMAS = SK_CHUNK * ROWS / 8;
  constexpr int S_DMAS = SK_CHUNK * ROWS * 2 / 64;
  auto stage = [&](int c0, int valid) {
#pragma unroll
    for (int u = 0; u < A_DMAS / 4; ++u) {
      const int q = u * 4 + wave;
      if (q * 8 / ROWS < valid) {
        const int fr = q * 8 + (lane >> 3);
        const int r = fr % ROWS;
        const uint32_t src = static_cast<uint32_t>(min(r, M - 1)) * kb + (kt0 + c0 + fr / ROWS) * 128u +
                             (((lane & 7) ^ (r & 7)) * 16);
        SK_DMA(A + src, smem + q * 1024, 16)
      }
    }
#pragma unroll
    for (int u = 0; u < (S_DMAS + 3) / 4; ++u) {
      const int q = u * 4 + wave;
      if (q < S_DMAS && q * 64 / (2 * ROWS) < valid) {
        const int d = q * 64 + lane;
        const int r = (d % (2 * ROWS)) >> 1;
        const int j = min(d / (2 * ROWS), valid - 1);
        const uint32_t src = static_cast<uint32_t>(min(r, M - 1)) * kq + (kt0 + c0 + j) * 8u + (d & 1) * 4;
        SK_DMA(SA + src, smem + A_BYTES + q * 256, 4)
      }
    }
  };

  // Fragment reads: row i of a 16-row group, chunk g + 4·ks through the XOR.
  const int a_rd = i * 128 + ((g ^ (i & 7)) * 16);  // + (step·ROWS + 16mt)·128; ks = 1 is ^ 64
  const int sa_rd = A_BYTES + i * 8;                // + (step·ROWS + 16mt)·8
  // v_perm_b32 selector: byte g of the low dword, byte g of the high one (= byte 4+g), two zero bytes (0x0c).
  const uint32_t sel = 0x0c0c0400u + g * 0x0101u;

#define SK_MFMA_KS(ks) /* op_sel is an immediate */                                                        \
  _Pragma("unroll") for (int mt = 0; mt < MT; ++mt)                                                        \
  _Pragma("unroll") for (int nt = 0; nt < 2; ++nt)                                                         \
    acc[mt][nt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(                                        \
        p4_operand(bq[slot][nt * 2 + ks]), p4_operand(af[mt][ks]), acc[mt][nt], 4, 4, ks, sb_[nt], ks, sa_[mt]);

  f32x4 acc[MT][2];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int d = 0; d < SK_DEPTH; ++d) SK_LOAD_B(d, d)

  for (int c0 = 0; c0 < nsteps; c0 += SK_CHUNK) {
    const int valid = min(SK_CHUNK, nsteps - c0);
    if (c0) __builtin_amdgcn_s_barrier();  // every wave has consumed the previous chunk
    stage(c0, valid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int j = 0; j < SK_CHUNK; ++j) {
      if (j >= valid) break;
      const int slot = j % SK_DEPTH;
      i32x4 af[MT][2];
      int sa_[MT], sb_[2];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const unsigned char* row_ = smem + (j * ROWS + 16 * mt) * 128 + a_rd;
        af[mt][0] = *reinterpret_cast<const i32x4*>(row_);
        af[mt][1] = *reinterpret_cast<const i32x4*>(smem + (j * ROWS + 16 * mt) * 128 + (a_rd ^ 64));
        const u32x2 raw = *reinterpret_cast<const u32x2*>(smem + (j * ROWS + 16 * mt) * 8 + sa_rd);
        sa_[mt] = __builtin_amdgcn_perm(raw[1], raw[0], sel);
      }
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) sb_[nt] = __builtin_amdgcn_perm(sb_raw[slot][nt][1], sb_raw[slot][nt][0], sel);
      // (B, A): a lane holds row m = 16mt + i, columns 16nt + 4g .. +3. First scale operand B's, second A's.
      SK_MFMA_KS(0)
      SK_MFMA_KS(1)
      SK_LOAD_B(slot, c0 + j + SK_DEPTH)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#undef SK_LOAD_B
#undef SK_DMA
#undef SK_MFMA_KS

#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int row = 16 * mt + i;
    if (row >= M) continue;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int col = n0 + 32 * wave + 16 * nt + 4 * g;
      const f32x4 v = acc[mt][nt];
      if (W == nullptr)
        *reinterpret_cast<u32x2*>(C + static_cast<size_t>(row) * N + col) =
            u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
      else
        *reinterpret_cast<f32x4*>(W + (static_cast<size_t>(blockIdx.y) * M + row) * N + col) = v;
    }
  }
}

// One thread per four consecutive columns: split fp32 loads of 16 bytes, summed
// in ascending s, one 8-byte bf16 store. mn4 = M·N/4.
__global__ __launch_bounds__(256) void mxfp4_skinny_reduce(const f32x4* __restrict__ W, u32x2* __restrict__ C,
                                                           int split, size_t mn4) {
  const size_t t = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= mn4) return;
  f32x4 s = W[t];
  for (int p = 1; p < split; ++p) s += W[p * mn4 + t];
  C[t] = u32x2{pack_bf16x2(s[0], s[1]), pack_bf16x2(s[2], s[3])};
}

bool g_skinny_attr[4] = {false, false, false, false};

template <int MT>
const char* launch_skinny_mt(const uint8_t* a, const uint8_t* b, const uint8_t* sa, const uint8_t* sb, uint16_t* c,
                             float* w, int m, int n, int k, int split, hipStream_t stream) {
  auto kernel = gemm_mxfp4_skinny<MT>;
  if (!g_skinny_attr[MT - 1]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            sk_lds(MT)) != hipSuccess)
      return "gemm_mxfp4_skinny_nt: cannot reserve LDS";
    g_skinny_attr[MT - 1] = true;
  }
  hipLaunchKernelGGL(kernel, dim3(n / 128, split), dim3(SK_THREADS), sk_lds(MT), stream, a, b, sa, sb, c, w, m, n, k,
                     k / 256 / split);
  return nullptr;
}

const char* launch_gemm_mxfp4_skinny(const void* a, const void* b, const void* sa, const void* sb, void* c, int m,
                                     int n, int k, int split, void* ws, unsigned long long ws_bytes,
                                     hipStream_t stream) {
  if (m < 1 || m > 64 || n <= 0 || k <= 0 || n % 128 || k % 256 || split < 1 || split > 65535 || (k / 256) % split ||
      static_cast<uint64_t>(n) * (k / 2) >= (1ull << 32))
    return "gemm_mxfp4_skinny_nt: needs 1 <= M <= 64, N a multiple of 128, K of 256, split_k dividing K/256 (at most "
           "65535), N*K/2 < 2^32";
  if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15)
    return "gemm_mxfp4_skinny_nt: A, B and C must be 16-byte aligned";
  if (sa == nullptr || sb == nullptr) return "gemm_mxfp4_skinny_nt: both scale tensors are required";
  if ((reinterpret_cast<uintptr_t>(sa) | reinterpret_cast<uintptr_t>(sb)) & 3)
    return "gemm_mxfp4_skinny_nt: scales must be 4-byte aligned";
  const size_t mn = static_cast<size_t>(m) * n;
  if (split > 1) {
    if (ws == nullptr || (reinterpret_cast<uintptr_t>(ws) & 15))
      return "gemm_mxfp4_skinny_nt: split_k > 1 needs a 16-byte aligned workspace";
    if (ws_bytes < static_cast<unsigned long long>(split) * mn * 4)
      return "gemm_mxfp4_skinny_nt: workspace smaller than split_k*M*N*4 bytes";
  }
  const uint8_t* a8 = static_cast<const uint8_t*>(a);
  const uint8_t* b8 = static_cast<const uint8_t*>(b);
  const uint8_t* sa8 = static_cast<const uint8_t*>(sa);
  const uint8_t* sb8 = static_cast<const uint8_t*>(sb);
  uint16_t* c16 = static_cast<uint16_t*>(c);
  float* w = split > 1 ? static_cast<float*>(ws) : nullptr;
  const char* err = nullptr;
  switch ((m + 15) / 16) {
    case 1: err = launch_skinny_mt<1>(a8, b8, sa8, sb8, c16, w, m, n, k, split, stream); break;
    case 2: err = launch_skinny_mt<2>(a8, b8, sa8, sb8, c16, w, m, n, k, split, stream); break;
    case 3: err = launch_skinny_mt<3>(a8, b8, sa8, sb8, c16, w, m, n, k, split, stream); break;
    default: err = launch_skinny_mt<4>(a8, b8, sa8, sb8, c16, w, m, n, k, split, stream); break;
  }
  if (err) return err;
  if (split > 1)
    hipLaunchKernelGGL(mxfp4_skinny_reduce, dim3(static_cast<unsigned>((mn / 4 + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const f32x4*>(w), reinterpret_cast<u32x2*>(c16), split, mn / 4);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

PyObject* py_gemm_mxfp4_skinny(PyObject*, PyObject* args) {
  unsigned long long a, b, sa, sb, c, ws, ws_bytes, stream;
  int m, n, k, split;
  if (!PyArg_ParseTuple(args, "KKKKKiiiiKKK", &a, &b, &sa, &sb, &c, &m, &n, &k, &split, &ws, &ws_bytes, &stream))
    return nullptr;
  const char* err = launch_gemm_mxfp4_skinny(reinterpret_cast<void*>(a), reinterpret_cast<void*>(b),
                                             reinterpret_cast<void*>(sa), reinterpret_cast<void*>(sb),
                                             reinterpret_cast<void*>(c), m, n, k, split, reinterpret_cast<void*>(ws),
                                             ws_bytes, reinterpret_cast<hipStream_t>(stream));
  if (err) {
    PyErr_SetString(PyExc_RuntimeError, err);
    return nullptr;
  }
  Py_RETURN_NONE;
}

constexpr const char* kSkinnyDoc =
    "gemm_mxfp4_skinny_nt(a, b, scale_a, scale_b, c, M, N, K, split_k, workspace, workspace_bytes, stream): the "
    "gemm_mxfp4_nt product for 1 <= M <= 64, N a multiple of 128, K of 256, K split over split_k blocks; fp32 "
    "partials in workspace (split_k*M*N*4 bytes) reduced in order when split_k > 1.";
