// The scattered epilogue of the tiled bf16 GEMMs, straight from the accumulators: ONE copy of its
// bounds tests, #included as the tail of gemm_kernel (gemm.hip), gemm_big_kernel (gemm_big.hip) and
// g256::store_tile (gemm256_tile.h). A code fragment, not a header: no include guard, no namespace.
// (gemm.hip writes its split-K slabs itself, ahead of the include; see the comment there.)
//
// Why text and not a function: a __forceinline__ store_scatter<NI, NJ, OUT_MODE>(p, acc, ...) was
// built first. hipcc optimises such a helper on its own before it inlines it (with p and acc behind
// pointers), and the result is not re-derived afterwards: every instantiation of all three kernels
// changed, the full epilogues by ~5 % of their instructions (docs/PERFORMANCE.md, "GEMM sources:
// one copy of the shared pieces"). As text the compiler sees what it saw when the copies were
// separate, and the instruction streams are the parent's.
//
// In scope where it is included:
//   NI, NJ     constexpr int: the accumulator's fragment grid (4 x 4 for the 64x64 wave tiles of
//              gemm.hip / gemm_big.hip, 8 x WN/16 in the 256-row kernels)
//   OUT_MODE   0 = bf16 output, 1 = fp32 output, both with alpha, beta * C, bf16 / fp32 bias,
//              pre-activation store to Z and activation; 2 = fp32 split-K partial into slab z of the
//              workspace (alpha only; [M][N] slabs, ldc = N)
//   p          GemmArgs;  acc  f32x4[NI][NJ], acc[i][j][r] = C[mrow + 16 i][ncol + 16 j + r] (the
//              MFMA operands are swapped so that a lane owns 4 consecutive columns)
//   mrow, ncol this lane's first row / column;  b, z  batch index and blockIdx.y
// A quad of columns leaves as one ushort4 / float4 where the row alignment allows (vec_ok) and the
// quad is whole, else element by element inside N. It returns from the enclosing function.
  if (OUT_MODE == 2) {
    float* W = p.ws + (int64_t)z * p.M * p.N;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int m = mrow + i * 16;
      if (m >= p.M) continue;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int n = ncol + j * 16;
        float* dst = W + (int64_t)m * p.N + n;
        if (n + 3 < p.N && (p.N & 3) == 0) {
          *reinterpret_cast<float4*>(dst) = make_float4(acc[i][j][0] * p.alpha, acc[i][j][1] * p.alpha,
                                                        acc[i][j][2] * p.alpha, acc[i][j][3] * p.alpha);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) if (n + r < p.N) dst[r] = acc[i][j][r] * p.alpha;
        }
      }
    }
    return;
  }
  typedef typename std::conditional<OUT_MODE == 0, bf16_t, float>::type OutT;
  OutT* C = reinterpret_cast<OutT*>(p.C) + (int64_t)b * p.sC;
  bf16_t* Zp = p.Z ? reinterpret_cast<bf16_t*>(p.Z) + (int64_t)b * p.sC : nullptr;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int m = mrow + i * 16;
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int n = ncol + j * 16;
      if (n >= p.N) continue;
      float v[4];
      const bool full = p.vec_ok && (n + 3 < p.N);
      OutT* dst = C + (int64_t)m * p.ldc + n;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = acc[i][j][r] * p.alpha;
        if (p.beta != 0.f && n + r < p.N) x += p.beta * Cvt<OutT>::to_f(dst[r]);
        if (p.bias && n + r < p.N)
          x += p.bias_bf16 ? bf2f(((const bf16_t*)p.bias)[n + r]) : ((const float*)p.bias)[n + r];
        v[r] = x;
      }
      if (Zp) {
        bf16_t* zd = Zp + (int64_t)m * p.ldc + n;
        if (full) {
          ushort4 o; o.x = f2bf(v[0]); o.y = f2bf(v[1]); o.z = f2bf(v[2]); o.w = f2bf(v[3]);
          *reinterpret_cast<ushort4*>(zd) = o;
        } else {
          for (int r = 0; r < 4; ++r) if (n + r < p.N) zd[r] = f2bf(v[r]);
        }
      }
      if (p.act != ACT_NONE) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = act_fwd(p.act, v[r]);
      }
      if (full) {
        if (OUT_MODE == 0) {
          ushort4 o; o.x = f2bf(v[0]); o.y = f2bf(v[1]); o.z = f2bf(v[2]); o.w = f2bf(v[3]);
          *reinterpret_cast<ushort4*>(dst) = o;
        } else {
          *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) if (n + r < p.N) dst[r] = Cvt<OutT>::from_f(v[r]);
      }
    }
  }
