// FP8 KV cache (gfx950 / CDNA4): the kernel that fills it and decode attention
// over it. Part of workload.hip: included inside its anonymous namespace after
// attn_prefill.h. The grid, the per-sequence slices, the workspace layout and
// attn_decode_combine are attn_decode.h's, used unchanged; how the bytes move
// is new, because a cached row is 128 bytes of e4m3 instead of 256 of bf16.
// Launchers, checks and the Python bindings are at the bottom.
//
// Cache. k_cache, v_cache [B,Hkv,S_max,128] OCP e4m3 ("fn"); k_scale, v_scale
// [B,Hkv,S_max] E8M0 bytes: row s of head h means e4m3 · 2^(byte − 127).
// S_max % 4 == 0. 129 bytes per cached row where the bf16 cache has 256.
//
//   kv_append_fp8    rows of k_new, v_new [B,Sq,Hkv,128] bf16 → the caches at
//                    position seq_lens[b] − Sq + i (rows of negative position
//                    are left padding and skipped, as are positions ≥ S_max).
//                    Per row, with e the exponent field of amax as a float:
//                    scale byte = max(e − 8 + bump, 1), bump = 1 where the
//                    mantissa of amax exceeds 1.75 (amax·2^−X > 448 ⇔ 1.m·256 >
//                    448); amax = 0 gives 127. 2^−X is the float of exponent
//                    field 254 − byte (7..253: normal), so scaling is an exact
//                    multiply and no product exceeds 448: v_cvt_pk_fp8_f32 (RNE)
//                    never saturates. 16 lanes per row, 16 bytes in and 8 out
//                    per lane, amax by four xor-shuffles, the scale byte stored
//                    by the group's first lane. Grid (⌈rows/16⌉, 2): y picks K or V.
//   attn_decode_fp8  out[b,h,:] = Σ_s softmax_s(scale·q[b,h,:]·k[b,g,s,:]) · v[b,g,s,:]
//                    over s < seq_lens[b] on the dequantised cache; bf16 MFMA
//                    operands, fp32 softmax and accumulation as attn_decode.
//
// Work split. Grid (Hkv, B, split_kv), 256 threads, as attn_decode, with
// AF_TILE = 64 keys per wave tile: half the bytes per key, so twice the keys
// keep the same 8 KiB of K in the register ring and 8 KiB of V per LDS
// buffer, the bytes in flight per wave of the bf16 kernel. Wave w walks tiles
// w, w+4, … of the block's slice; no block barrier in the loop.
//
// Lanes. i = lane & 15, g = lane >> 4; v_mfma_f32_16x16x32_bf16 as in
// attn_decode.h. Sub-tile t (0..3) of a tile holds, in MFMA row ρ, key
// kv0 + 16(ρ/4) + 4t + ρ%4, so that lane (i, g) ends with the scores of head i
// at keys kv0 + 16g + 4t + r, r = 0..3: over t, sixteen consecutive keys.
//
// K, HBM → registers → MFMA, no LDS. The contraction is permuted so that a
// lane loads contiguous bytes: lane (i, g) loads the 32 bytes at 32g of its
// key row as two dwordx4, and MFMA step ks takes bytes 8ks..8ks+7, d = 32g +
// 8ks + 0..7; Q's fragment of step ks is the 16 bytes of bf16 at the same d,
// loaded once. Eight bytes become eight bf16 with four
// v_cvt_scalef32_pk_bf16_fp8, measured on the device to give bytes 0,1
// (word 0) or 2,3 (word 1) in order, times the power of two of the scale
// operand's exponent. (v_cvt_pk_f32_fp8 plus v_cvt_pk_bf16_f32 is twice the
// instructions.)
//
// K's scale rides in that conversion: the operand is float(byte << 23) of the
// lane's key row, one byte load per sub-tile (four per tile) and one shift,
// where scaling the four fp32 scores of a sub-tile takes four extractions and
// four multiplies. Exact while e4m3·2^k stays in bf16's normal range, which
// has fp32's exponent. Row and byte are clamped to len − 1 past the end, so
// the byte is always one that kv_append_fp8 wrote.
//
// V, LDS-DMA + transposing read. A wave stages its tile (64 rows × 128 bytes)
// with eight global_load_lds_dwordx4 into its private double buffer: 64 KiB
// per block, two blocks per CU. DMA q writes LDS bytes [1024q, +1024), rows
// 8q .. 8q+7; lane l covers row r = 8q + l/8, physical 16-byte chunk l%8,
// loaded from logical chunk (l%8) ^ f(r), f(r) = (r/2)%4 + 4·((r/16)%2): the
// swizzle is on the source address because the DMA writes LDS lane-linearly.
// ds_read_b64_tr_b8 gives lane i of a 16-lane group, as element e, byte i%8 of
// the 8 bytes addressed by lane 2e + i/8 of the group (read off the device
// with a one-wave probe, pinned by the one-hot test). Lane j of group g
// addresses row 16g + 8u + j/2, logical bytes 16db + 8(j%2), so lane i
// receives V[kv0 + 16g + 8u + e][16db + i]: k-slot 8g + e of output MFMA u
// (u = 0, 1: 32 keys each) is key kv0 + 16g + 8u + e, exactly the order in
// which the lane holds P from sub-tiles 2u and 2u+1. P goes from the score
// accumulator to the operand in registers, no LDS and no cross-lane move.
// Bank conflicts: a b64 read is served in two halves of 32 lanes × 8 bytes =
// all 64 banks once. A half covers g ∈ {0,1} or {2,3}: rows 8u+e and 16+8u+e
// (+32), sixteen rows. Rows are 128 bytes, so a row's parity picks the half
// of the 256-byte bank space, and among the eight rows of one parity f takes
// eight different values ((r/2)%4 separates e, (r/16)%2 separates g): sixteen
// different 16-byte slots, each read by two lanes 8 bytes apart. Unswizzled,
// the eight rows of one parity would share one slot: 8-way.
//
// V's scale runs along the contraction and is folded into P:
// p' = bf16(p · 2^(vs − 127)), which is bf16(p)·2^(vs − 127) exactly; the
// running sum adds bf16(p) as in the bf16 kernel. A lane's four keys of a
// sub-tile are one dword of v_scale (S_max % 4 == 0), read at
// min(key, S_max − 4): a dword moved by the clamp holds only keys ≥ S_max.
// Keys at or past len get score −inf and p' selected to 0, not multiplied:
// their scale bytes may be anything, 0 · inf would be NaN.
//
// Waits. Iteration j issues, after the score MFMAs of tile j: K of tile j+2
// (8 dwordx4 + 4 scale bytes) and V's scales of tile j+2 (4 dwords) into the
// register ring slot that tile j has just left (slot = parity, static: the
// loop is unrolled by two), then the 8 DMAs of tile j+1 into the other buffer
// (whose reads, of tile j−1, have been waited for), 24 in all, the same past
// the wave's last tile (clamped rows, never used). Every register load is two
// tiles ahead of its use, so the vmcnt(0) that the compiler puts before the
// score MFMAs of every even tile (as in attn_decode) is the only one it adds.
// Then s_waitcnt vmcnt(24): what may remain in flight is exactly those 24, so
// tile j's V, issued before them, has landed. No barrier; a
// wrong count shows as stale data in the tests. The transposing reads are
// inline assembly with their own lgkmcnt wait, for attn_decode.h's reason.
//
// End: attn_decode's. vmcnt(0), barrier, the four waves' states merged in
// wave order over the V buffers; split_kv > 1 stores the partial in
// attn_decode's workspace layout and attn_decode_combine finishes.
//
// Measured on the MI355X: profiles/attn_decode_fp8_ab.md.

constexpr int AF_TILE = 64;                    // keys per wave tile
constexpr int AF_LDS = 4 * 2 * AF_TILE * 128;  // 4 waves × double buffer × 8 KiB

// Eight e4m3 bytes (lo: 0..3, hi: 4..7) times 2^(exponent of scale − 127) → eight bf16, in order.
__device__ __forceinline__ bf16x8 af_cvt8(uint32_t lo, uint32_t hi, float scale) {
  const int a = static_cast<int>(lo), b = static_cast<int>(hi);
  return __builtin_bit_cast(
      bf16x8, (u32x4){__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, scale, false)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, scale, true)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, scale, false)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, scale, true))});
}

// 2^(byte − 127) for E8M0 byte `idx` of a scale dword; exact for bytes 1..254.
__device__ __forceinline__ float af_scale(uint32_t dword, int idx) {
  return __builtin_bit_cast(float, ((dword >> (8 * idx)) & 0xffu) << 23);
}

__global__ __launch_bounds__(AD_THREADS) void attn_decode_fp8(
    const uint16_t* __restrict__ Q, const unsigned char* __restrict__ K, const unsigned char* __restrict__ V,
    const unsigned char* __restrict__ KS, const unsigned char* __restrict__ VS, const int* __restrict__ seq_lens,
    uint16_t* __restrict__ O, float* __restrict__ W, int G, int s_max, float scale) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15;
  const int g = lane >> 4;
  const int hk = blockIdx.x, b = blockIdx.y, z = blockIdx.z;
  const int Hkv = gridDim.x, B = gridDim.y, split = gridDim.z;
  const int Hq = Hkv * G;

  const int len = min(max(seq_lens[b], 0), s_max);
  const int last = max(len - 1, 0);  // the row that out-of-range keys load
  const int tiles = (len + AF_TILE - 1) / AF_TILE;
  const int per = (tiles + split - 1) / split;
  const int t0 = z * per + wave;                  // this wave's first tile
  const int t1 = min((z + 1) * per, tiles);       // end of the block's slice
  const int n = t1 > t0 ? (t1 - t0 + 3) / 4 : 0;  // this wave's tiles: t0 + 4j
  const uint32_t row0 = static_cast<uint32_t>(b * Hkv + hk) * static_cast<uint32_t>(s_max);  // first row of this head
  const uint32_t base = row0 * 128u;
  const float sc = scale * 1.44269504088896340736f;

  // Q fragments: head min(i, G−1) of the group, the 16 bytes of d = 32g + 8ks + 0..7.
  bf16x8 qf[4];
  {
    const uint16_t* qrow = Q + (static_cast<size_t>(b) * Hq + hk * G + min(i, G - 1)) * 128 + 32 * g;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qrow + 8 * ks);
  }

  i32x4 kf[2][8];      // [slot][2t + half]: bytes 32g + 16·half .. +15 of sub-tile t's key row
  uint32_t ksb[2][4];  // [slot][t]: that row's scale byte
  uint32_t vsd[2][4];  // [slot][t]: v_scale of keys kv0 + 16g + 4t + 0..3
  const int krow = 16 * (i >> 2) + (i & 3);
  auto load_k = [&](i32x4(&dst)[8], uint32_t(&sb)[4], int j) {
    const int kv0 = (t0 + 4 * j) * AF_TILE;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint32_t row = static_cast<uint32_t>(min(kv0 + krow + 4 * t, last));
      const uint32_t off = base + row * 128u + 32 * g;
      dst[2 * t] = *reinterpret_cast<const i32x4*>(K + off);
      dst[2 * t + 1] = *reinterpret_cast<const i32x4*>(K + off + 16);
      sb[t] = KS[row0 + row];
    }
  };
  auto load_vs = [&](uint32_t(&dst)[4], int j) {
    const int kv0 = (t0 + 4 * j) * AF_TILE;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      dst[t] = *reinterpret_cast<const uint32_t*>(VS + row0 + min(kv0 + 16 * g + 4 * t, s_max - 4));
  };
  unsigned char* const vbuf = smem + wave * (2 * AF_TILE * 128);
  auto stage_v = [&](int buf, int j) {
    const int kv0 = (t0 + 4 * j) * AF_TILE;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int r = 8 * q + (lane >> 3);  // lane l: row 8q + l/8, physical chunk l%8
      const int f = ((r >> 1) & 3) | (((r >> 4) & 1) << 2);
      const uint32_t src = base + static_cast<uint32_t>(min(kv0 + r, last)) * 128u + (((lane & 7) ^ f) << 4);
      __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)(V + src),
                                       (__attribute__((address_space(3))) void*)(vbuf + buf * (AF_TILE * 128) + q * 1024),
                                       16, 0, 0);
    }
  };
  // Transposing reads: lane j = i of group g addresses row 16g + 8u + j/2, bytes 16·(db ^ f(row)) + 8(j%2);
  // f is the same for u = 0 and 1 (row + 8 changes neither (r/2)%4 nor (r/16)%2).
  const int rd_row = 16 * g + (i >> 1);
  const int rd_f = ((rd_row >> 1) & 3) | (((rd_row >> 4) & 1) << 2);
  uint32_t rd_addr[8];  // LDS address of this lane's 8 bytes for u = 0 of buffer 0, per db
#pragma unroll
  for (int db = 0; db < 8; ++db)
    rd_addr[db] = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(
                      (__attribute__((address_space(3))) unsigned char*)(vbuf))) +
                  rd_row * 128 + ((db ^ rd_f) << 4) + ((i & 1) << 3);

  float m = AD_NEG_INF, l = 0.f;
  f32x4 acc[8];
#pragma unroll
  for (int db = 0; db < 8; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto step = [&](auto slot_c, int j) {
    constexpr int slot = decltype(slot_c)::value;
    const int kv0 = (t0 + 4 * j) * AF_TILE;
    f32x4 s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      const float kscale = __builtin_bit_cast(float, ksb[slot][t] << 23);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const i32x4 raw = kf[slot][2 * t + (ks >> 1)];
        s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af_cvt8(static_cast<uint32_t>(raw[2 * (ks & 1)]), static_cast<uint32_t>(raw[2 * (ks & 1) + 1]), kscale),
            qf[ks], s[t], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    const uint32_t vs[4] = {vsd[slot][0], vsd[slot][1], vsd[slot][2], vsd[slot][3]};
    load_k(kf[slot], ksb[slot], j + 2);
    load_vs(vsd[slot], j + 2);
    stage_v(slot ^ 1, j + 1);
    __builtin_amdgcn_sched_barrier(0);

    float mt = AD_NEG_INF;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] = kv0 + 16 * g + 4 * t + r < len ? s[t][r] * sc : AD_NEG_INF;
        mt = fmaxf(mt, s[t][r]);
      }
    mt = fmaxf(mt, __shfl_xor(mt, 16));
    mt = fmaxf(mt, __shfl_xor(mt, 32));
    const float m_new = fmaxf(m, mt);
    const float m_ref = m_new == AD_NEG_INF ? 0.f : m_new;  // nothing seen yet: exp2(−inf − 0) = 0, never −inf − −inf
    if (__any(m_new > m)) {
      const float alpha = m_new > m ? __builtin_amdgcn_exp2f(m - m_ref) : 1.f;
      l *= alpha;
#pragma unroll
      for (int db = 0; db < 8; ++db) acc[db] *= alpha;
    }
    m = m_new;
    uint32_t pk[8];  // [2t + h]: p' of keys kv0 + 16g + 4t + 2h, +1
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float p0 = __builtin_amdgcn_exp2f(s[t][2 * h] - m_ref);
        const float p1 = __builtin_amdgcn_exp2f(s[t][2 * h + 1] - m_ref);
        const uint32_t u = pack_bf16x2(p0, p1);
        l += __builtin_bit_cast(float, u << 16) + __builtin_bit_cast(float, u & 0xffff0000u);
        const int key = kv0 + 16 * g + 4 * t + 2 * h;
        pk[2 * t + h] = pack_bf16x2(key < len ? p0 * af_scale(vs[t], 2 * h) : 0.f,
                                    key + 1 < len ? p1 * af_scale(vs[t], 2 * h + 1) : 0.f);
      }
    const bf16x8 pf[2] = {__builtin_bit_cast(bf16x8, (u32x4){pk[0], pk[1], pk[2], pk[3]}),
                          __builtin_bit_cast(bf16x8, (u32x4){pk[4], pk[5], pk[6], pk[7]})};

    // V of tile j has landed once only the 24 loads and DMAs issued above remain.
    asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    u32x2 vf[8][2];  // [db][u]
#pragma unroll
    for (int hb = 0; hb < 8; hb += 4) {
      asm volatile(
          "ds_read_b64_tr_b8 %0, %8 offset:%12\n\tds_read_b64_tr_b8 %1, %8 offset:%13\n\t"
          "ds_read_b64_tr_b8 %2, %9 offset:%12\n\tds_read_b64_tr_b8 %3, %9 offset:%13\n\t"
          "ds_read_b64_tr_b8 %4, %10 offset:%12\n\tds_read_b64_tr_b8 %5, %10 offset:%13\n\t"
          "ds_read_b64_tr_b8 %6, %11 offset:%12\n\tds_read_b64_tr_b8 %7, %11 offset:%13\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(vf[hb][0]), "=&v"(vf[hb][1]), "=&v"(vf[hb + 1][0]), "=&v"(vf[hb + 1][1]), "=&v"(vf[hb + 2][0]),
            "=&v"(vf[hb + 2][1]), "=&v"(vf[hb + 3][0]), "=&v"(vf[hb + 3][1])
          : "v"(rd_addr[hb]), "v"(rd_addr[hb + 1]), "v"(rd_addr[hb + 2]), "v"(rd_addr[hb + 3]),
            "n"(slot * (AF_TILE * 128)), "n"(slot * (AF_TILE * 128) + 8 * 128)
          : "memory");
#pragma unroll
      for (int db = hb; db < hb + 4; ++db)
#pragma unroll
        for (int u = 0; u < 2; ++u)
          acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af_cvt8(vf[db][u][0], vf[db][u][1], 1.f), pf[u], acc[db],
                                                            0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  if (n > 0) {
    load_k(kf[0], ksb[0], 0);
    load_k(kf[1], ksb[1], 1);
    load_vs(vsd[0], 0);
    load_vs(vsd[1], 1);
    stage_v(0, 0);
    __builtin_amdgcn_sched_barrier(0);
    for (int j = 0; j < n; j += 2) {
      step(std::integral_constant<int, 0>{}, j);
      if (j + 1 >= n) break;
      step(std::integral_constant<int, 1>{}, j + 1);
    }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);

  // Merge the four waves' states in wave order, over the V buffers (attn_decode's end, same LDS map).
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int db = 0; db < 8; ++db) *reinterpret_cast<f32x4*>(smem + wave * 8192 + db * 1024 + lane * 16) = acc[db];
  *reinterpret_cast<f32x2*>(smem + 32768 + wave * 512 + lane * 8) = f32x2{m, l};
  __syncthreads();
  float f[4], M = AD_NEG_INF, L = 0.f;
#pragma unroll
  for (int v = 0; v < 4; ++v) M = fmaxf(M, reinterpret_cast<const f32x2*>(smem + 32768 + v * 512 + lane * 8)[0][0]);
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const f32x2 ml = *reinterpret_cast<const f32x2*>(smem + 32768 + v * 512 + lane * 8);
    f[v] = ml[0] == AD_NEG_INF ? 0.f : __builtin_amdgcn_exp2f(ml[0] - M);
    L += ml[1] * f[v];
  }
  const size_t row = static_cast<size_t>(b) * Hq + hk * G + i;  // stored only where i < G
  const size_t rows = static_cast<size_t>(B) * Hq;
  const float inv = L > 0.f ? 1.f / L : 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int db = 2 * wave + u;
    f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int v = 0; v < 4; ++v) o += f[v] * *reinterpret_cast<const f32x4*>(smem + v * 8192 + db * 1024 + lane * 16);
    if (i >= G) continue;
    const int d = 16 * db + 4 * g;
    if (W == nullptr) {
      o *= inv;
      *reinterpret_cast<u32x2*>(O + row * 128 + d) = u32x2{pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
    } else {
      *reinterpret_cast<f32x4*>(W + (z * rows + row) * 128 + d) = o;
    }
  }
  if (W != nullptr && wave == 0 && g == 0 && i < G)
    *reinterpret_cast<f32x2*>(W + static_cast<size_t>(split) * rows * 128 + (z * rows + row) * 2) = f32x2{M, L};
}

// 16 lanes per row of 128 bf16; blockIdx.y = 0 quantises k_new into the K cache, 1 v_new into the V cache.
__global__ __launch_bounds__(256) void kv_append_fp8(const u32x4* __restrict__ k_new, const u32x4* __restrict__ v_new,
                                                     u32x2* __restrict__ k_cache, u32x2* __restrict__ v_cache,
                                                     uint8_t* __restrict__ k_scale, uint8_t* __restrict__ v_scale,
                                                     const int* __restrict__ seq_lens, int sq, int hkv, int s_max,
                                                     size_t rows) {
  const u32x4* src = blockIdx.y ? v_new : k_new;
  u32x2* cache = blockIdx.y ? v_cache : k_cache;
  uint8_t* scales = blockIdx.y ? v_scale : k_scale;
  const size_t row = static_cast<size_t>(blockIdx.x) * 16 + (threadIdx.x >> 4);  // (b, i, h) of [B,Sq,Hkv]
  const int c = threadIdx.x & 15;
  // A row's 16 lanes are live or not together; dead lanes stay active for the shuffles and skip the memory accesses.
  bool live = row < rows;
  size_t dst = 0;  // cache row
  if (live) {
    const size_t bi = row / hkv;
    const size_t bb = bi / sq;
    const long long pos = static_cast<long long>(seq_lens[bb]) - sq + static_cast<long long>(bi % sq);
    live = pos >= 0 && pos < s_max;
    dst = (bb * hkv + row % hkv) * static_cast<size_t>(s_max) + static_cast<size_t>(live ? pos : 0);
  }
  const u32x4 raw = live ? src[row * 16 + c] : u32x4{0, 0, 0, 0};
  float v[8];
  uint32_t amax = 0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const uint32_t lo = raw[p] << 16, hi = raw[p] & 0xffff0000u;  // bf16 → fp32 is a shift
    v[2 * p] = __builtin_bit_cast(float, lo);
    v[2 * p + 1] = __builtin_bit_cast(float, hi);
    amax = max(amax, max(lo & 0x7fffffffu, hi & 0x7fffffffu));  // non-negative floats order as integers
  }
#pragma unroll
  for (int x = 1; x < 16; x <<= 1) amax = max(amax, static_cast<uint32_t>(__shfl_xor(static_cast<int>(amax), x)));
  const int e = static_cast<int>(amax >> 23);
  const int bump = (amax & 0x7fffffu) > 0x600000u;  // 1.m > 1.75: amax·2^−X would exceed 448
  const uint32_t sbyte = amax == 0 ? 127u : static_cast<uint32_t>(max(e - 8 + bump, 1));
  const float inv = __builtin_bit_cast(float, (254u - sbyte) << 23);
  int w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * inv, v[1] * inv, 0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * inv, v[3] * inv, w0, true);
  int w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[4] * inv, v[5] * inv, 0, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[6] * inv, v[7] * inv, w1, true);
  if (live) {
    cache[dst * 16 + c] = u32x2{static_cast<uint32_t>(w0), static_cast<uint32_t>(w1)};
    if (c == 0) scales[dst] = static_cast<uint8_t>(sbyte);
  }
}

bool g_attn_fp8_attr = false;

const char* launch_attn_decode_fp8(const void* q, const void* k, const void* v, const void* ks, const void* vs,
                                   const void* lens, void* out, int b, int hkv, int g, int s_max, float scale,
                                   int split, void* ws, unsigned long long ws_bytes, hipStream_t stream) {
  if (b < 1 || b > 65535 || hkv < 1 || s_max < 4 || s_max % 4 || split < 1 || split > 65535)
    return "attn_decode_fp8: needs 1 <= B <= 65535, Hkv >= 1, S_max a positive multiple of 4, 1 <= split_kv <= 65535";
  if (g < 1 || g > 16) return "attn_decode_fp8: needs 1 <= Hq/Hkv <= 16";
  if (static_cast<uint64_t>(b) * hkv * s_max * 128 >= (1ull << 32))
    return "attn_decode_fp8: a cache must be smaller than 2^32 bytes (B*Hkv*S_max*128)";
  if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
       reinterpret_cast<uintptr_t>(out)) & 15)
    return "attn_decode_fp8: q, k_cache, v_cache and out must be 16-byte aligned";
  if (ks == nullptr || vs == nullptr || lens == nullptr ||
      ((reinterpret_cast<uintptr_t>(ks) | reinterpret_cast<uintptr_t>(vs) | reinterpret_cast<uintptr_t>(lens)) & 3))
    return "attn_decode_fp8: k_scale, v_scale and seq_lens must be 4-byte aligned";
  const size_t rows = static_cast<size_t>(b) * hkv * g;
  if (split > 1) {
    if (ws == nullptr || (reinterpret_cast<uintptr_t>(ws) & 15))
      return "attn_decode_fp8: split_kv > 1 needs a 16-byte aligned workspace";
    if (ws_bytes < static_cast<unsigned long long>(split) * rows * 130 * 4)
      return "attn_decode_fp8: workspace smaller than split_kv*B*Hq*130*4 bytes";
  }
  if (!g_attn_fp8_attr) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(attn_decode_fp8), hipFuncAttributeMaxDynamicSharedMemorySize,
                            AF_LDS) != hipSuccess)
      return "attn_decode_fp8: cannot reserve LDS";
    g_attn_fp8_attr = true;
  }
  float* w = split > 1 ? static_cast<float*>(ws) : nullptr;
  uint16_t* o16 = static_cast<uint16_t*>(out);
  hipLaunchKernelGGL(attn_decode_fp8, dim3(hkv, b, split), dim3(AD_THREADS), AF_LDS, stream,
                     static_cast<const uint16_t*>(q), static_cast<const unsigned char*>(k),
                     static_cast<const unsigned char*>(v), static_cast<const unsigned char*>(ks),
                     static_cast<const unsigned char*>(vs), static_cast<const int*>(lens), o16, w, g, s_max, scale);
  if (split > 1)
    hipLaunchKernelGGL(attn_decode_combine, dim3(static_cast<unsigned>((rows * 32 + 255) / 256)), dim3(256), 0, stream,
                       static_cast<const float*>(w), o16, split, rows);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

const char* launch_kv_append_fp8(const void* k_new, const void* v_new, void* k, void* v, void* ks, void* vs,
                                 const void* lens, int b, int sq, int hkv, int s_max, hipStream_t stream) {
  if (b < 1 || sq < 1 || hkv < 1 || s_max < 1) return "kv_append_fp8: needs B, Sq, Hkv and S_max positive";
  const uint64_t rows = static_cast<uint64_t>(b) * sq * hkv;
  if (rows >= (1ull << 31) || static_cast<uint64_t>(b) * hkv * s_max >= (1ull << 40))
    return "kv_append_fp8: needs B*Sq*Hkv < 2^31 rows and B*Hkv*S_max < 2^40";
  if ((reinterpret_cast<uintptr_t>(k_new) | reinterpret_cast<uintptr_t>(v_new)) & 15)
    return "kv_append_fp8: k_new and v_new must be 16-byte aligned";
  if ((reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v)) & 7)
    return "kv_append_fp8: k_cache and v_cache must be 8-byte aligned";
  if (ks == nullptr || vs == nullptr || lens == nullptr || (reinterpret_cast<uintptr_t>(lens) & 3))
    return "kv_append_fp8: needs k_scale, v_scale and a 4-byte aligned seq_lens";
  hipLaunchKernelGGL(kv_append_fp8, dim3(static_cast<unsigned>((rows + 15) / 16), 2), dim3(256), 0, stream,
                     static_cast<const u32x4*>(k_new), static_cast<const u32x4*>(v_new), static_cast<u32x2*>(k),
                     static_cast<u32x2*>(v), static_cast<uint8_t*>(ks), static_cast<uint8_t*>(vs),
                     static_cast<const int*>(lens), sq, hkv, s_max, static_cast<size_t>(rows));
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

PyObject* py_attn_decode_fp8(PyObject*, PyObject* args) {
  unsigned long long q, k, v, ks, vs, lens, out, ws, ws_bytes, stream;
  int b, hkv, g, s_max, split;
  double scale;
  if (!PyArg_ParseTuple(args, "KKKKKKKiiiidiKKK", &q, &k, &v, &ks, &vs, &lens, &out, &b, &hkv, &g, &s_max, &scale,
                        &split, &ws, &ws_bytes, &stream))
    return nullptr;
  const char* err = launch_attn_decode_fp8(
      reinterpret_cast<void*>(q), reinterpret_cast<void*>(k), reinterpret_cast<void*>(v), reinterpret_cast<void*>(ks),
      reinterpret_cast<void*>(vs), reinterpret_cast<void*>(lens), reinterpret_cast<void*>(out), b, hkv, g, s_max,
      static_cast<float>(scale), split, reinterpret_cast<void*>(ws), ws_bytes, reinterpret_cast<hipStream_t>(stream));
  if (err) {
    PyErr_SetString(PyExc_RuntimeError, err);
    return nullptr;
  }
  Py_RETURN_NONE;
}

PyObject* py_kv_append_fp8(PyObject*, PyObject* args) {
  unsigned long long k_new, v_new, k, v, ks, vs, lens, stream;
  int b, sq, hkv, s_max;
  if (!PyArg_ParseTuple(args, "KKKKKKKiiiiK", &k_new, &v_new, &k, &v, &ks, &vs, &lens, &b, &sq, &hkv, &s_max, &stream))
    return nullptr;
  const char* err = launch_kv_append_fp8(reinterpret_cast<void*>(k_new), reinterpret_cast<void*>(v_new),
                                         reinterpret_cast<void*>(k), reinterpret_cast<void*>(v),
                                         reinterpret_cast<void*>(ks), reinterpret_cast<void*>(vs),
                                         reinterpret_cast<void*>(lens), b, sq, hkv, s_max,
                                         reinterpret_cast<hipStream_t>(stream));
  if (err) {
    PyErr_SetString(PyExc_RuntimeError, err);
    return nullptr;
  }
  Py_RETURN_NONE;
}

constexpr const char* kAttnDecodeFp8Doc =
    "attn_decode_fp8(q, k_cache, v_cache, k_scale, v_scale, seq_lens, out, B, Hkv, G, S_max, scale, split_kv, "
    "workspace, workspace_bytes, stream): attn_decode_bf16 over an e4m3 KV cache [B,Hkv,S_max,128] with one E8M0 "
    "scale byte per cached row [B,Hkv,S_max], S_max a multiple of 4; same workspace and split-KV merge.";
constexpr const char* kKvAppendFp8Doc =
    "kv_append_fp8(k_new, v_new, k_cache, v_cache, k_scale, v_scale, seq_lens, B, Sq, Hkv, S_max, stream): quantise "
    "bf16 rows [B,Sq,Hkv,128] to e4m3 with one power-of-two scale per row and write them at positions "
    "seq_lens[b] - Sq + i of the caches (negative positions are skipped).";
