// Fused LSTM cell of the fp32 engine (TrainConfig.compute_dtype = "fp32"): the reference's default network,
// BasicLSTMCell(256) unrolled over the rollout (game_ac_network.py:397-416, constants.py:30 USE_LSTM), with plain
// fp32 operands and every reduction in a FIXED order, like csrc/trunk_f32.hip.
//
// Same cell, batching and launch structure as csrc/lstm.hip / csrc/lstm_x3.hip (TF gate order i, j, f, o;
// forget_bias = 1; state reset by the previous step's done flag, by a select).  What changes is the operand format:
// x, h, c, the saved gates / [x | h] rows, dz and the kernel K are all fp32 and every GEMM runs on
// v_mfma_f32_16x16x4_f32, whose result is a k-ordered fmaf chain (one rounding per product).  It issues at 1/16 of
// the bf16 MFMA rate: this is the precision path, not the throughput path.
//   forward   z = [x | h] K + b       K read from the flat fp32 master directly (no operand copy, so no refresh
//   backward  [dx | dh_prev] = dz K^T launcher): k_off may be odd, so the loads from flat are scalar-width; each
//                                     32-wide k-step's 64 weight columns are staged once per workgroup in LDS
//   weight gradient dK = xh^T dz, db = column sums of dz over R = T*B rows: row chunks of LF32_CHUNK rows (the chunk
//             count depends on R alone), each chunk's partial dK / db stored to its own slab of a caller-provided
//             scratch buffer, then lstm_wgrad_reduce_f32 adds the slabs in chunk order into the flat gradient.  No
//             float atomics: one seed gives a bit-identical gradient run to run.
// The pointwise backward (launch_lstm_bwd_point, csrc/lstm.hip) and the state carry (launch_lstm_carry_f32,
// csrc/lstm_x3.hip) are fp32 in and out already and are shared.
// A 32-wide k chunk per lane group keeps the sibling kernels' load shape (csrc/trunk_f32.hip): lane group g = l>>4
// holds k = k0+8g .. k0+8g+7 and the chunk is eight 16x16x4 MFMAs, sub-step j feeding k-slot g with element
// k0+8g+j (A and B use the same permutation of k).  Four independent accumulators per wave cover the MFMA's
// 40-cycle dependent latency at its 32-cycle issue interval.
#include "common.h"

namespace lstmf32 {

#define LF32_CHUNK 4096                           // weight-gradient rows per partial slab
#define LF32_BSTR 66                              // LDS floats per staged k-row (64 + 2: lane groups 16 banks apart)

DEVI float sigm(float x) { return 1.f / (1.f + __expf(-x)); }
DEVI float tanh_f(float x) {
  const float e = __expf(-2.f * fabsf(x));
  const float t = (1.f - e) / (1.f + e);
  return copysignf(t, x);
}
DEVI void ld8(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
DEVI void st8(float* p, const float (&v)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
// one 32-wide k-step of a wave's 16 rows x 64 columns: a = the lane's 8 A values (k = 8*grp + j), Bt = the staged
// tile [k][column]
DEVI void mma_step(const float (&a)[8], const float* __restrict__ Bt, int grp, int c16, f4v (&acc)[4]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float* br = Bt + (8 * grp + j) * LF32_BSTR + c16;
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], br[g * 16], acc[g], 0, 0, 0);
  }
}

// ---------------------------------------------------------------------------
// forward: grid (ceil(B/64), H/16), 256 threads.  The workgroup owns 64 rows (wave w: rows 16w..16w+15) and the 4
// gate blocks of 16 units, so every lane finds the 4 gates of its unit in its own 4 accumulators and the cell
// update is the GEMM epilogue.  X: fp32 [B][ldx]; hprev / cprev fp32 [B][H]; K = flat + k_off, [F+H][4H].
// Staging role of thread tid: tile column tid & 63 (gate (tid&63)>>4, unit tid&15), k-rows (tid>>6) + 4 i.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lstm_fwd_f32_kernel(
    const float* __restrict__ X, int ldx, const float* __restrict__ hprev, const float* __restrict__ cprev,
    const uint8_t* __restrict__ prev_done, const float* __restrict__ flat, long k_off, long b_off,
    float* __restrict__ hout, float* __restrict__ cout, float* __restrict__ gates, float* __restrict__ xh, int F,
    int H, int B) {
  __shared__ float Bs[2][32 * LF32_BSTR];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int grp = l >> 4, c16 = l & 15;
  const int row0 = blockIdx.x * 64 + w * 16;
  const int ut = blockIdx.y;
  const int KK = F + H, G4 = 4 * H;
  const int arow = row0 + c16;
  const bool av = arow < B;
  const bool keep = av && !(prev_done && prev_done[arow]);
  const bool wr_xh = xh != nullptr && blockIdx.y == 0;
  const float* Kg = flat + k_off + (long)w * G4 + (l >> 4) * H + ut * 16 + (l & 15);
  float rb[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) rb[i] = Kg[(long)(4 * i) * G4];
  f4v acc[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) acc[g] = {0.f, 0.f, 0.f, 0.f};
  const int nsteps = KK / 32;
  for (int st = 0; st < nsteps; ++st) {
    const int buf = st & 1, k0 = st * 32;
#pragma unroll
    for (int i = 0; i < 8; ++i) Bs[buf][(w + 4 * i) * LF32_BSTR + l] = rb[i];
    __syncthreads();                              // this step's tile in LDS; the step before last is read out
    if (st + 1 < nsteps) {
#pragma unroll
      for (int i = 0; i < 8; ++i) rb[i] = Kg[(long)(k0 + 32 + 4 * i) * G4];
    }
    const int k = k0 + 8 * grp;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (av) {
      if (k < F) ld8(X + (long)arow * ldx + k, v);
      else if (keep) ld8(hprev + (long)arow * H + (k - F), v);
    }
    if (wr_xh && av) st8(xh + (long)arow * KK + k, v);
    mma_step(v, Bs[buf], grp, c16, acc);
  }
  if (row0 >= B) return;
  const int u = ut * 16 + c16;
  const float bi = flat[b_off + u], bj = flat[b_off + H + u], bff = flat[b_off + 2 * H + u],
              bo = flat[b_off + 3 * H + u];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + 4 * grp + r;
    if (row >= B) continue;
    const bool kp = !(prev_done && prev_done[row]);
    const float c0 = kp ? cprev[(long)row * H + u] : 0.f;
    const float si = sigm(acc[0][r] + bi);
    const float tj = tanh_f(acc[1][r] + bj);
    const float sf = sigm(acc[2][r] + bff + 1.0f);
    const float so = sigm(acc[3][r] + bo);
    const float c = c0 * sf + si * tj;
    const float h = tanh_f(c) * so;
    cout[(long)row * H + u] = c;
    hout[(long)row * H + u] = h;
    if (gates) {
      float* gr = gates + (long)row * 4 * H;
      gr[u] = si;
      gr[H + u] = tj;
      gr[2 * H + u] = sf;
      gr[3 * H + u] = so;
    }
  }
}

// ---------------------------------------------------------------------------
// backward GEMM: out[b][n] = sum_p dz[b][p] K[n][p]; n < F -> dx, n >= F -> dh_prev.  grid (ceil(B/64), (F+H)/64):
// a workgroup owns 64 rows (16 per wave) x 64 columns (4 blocks of 16).  K's rows are p-contiguous in flat, so the
// staging lanes run along p: thread tid loads p = tid & 31 of columns (tid>>5) + 8 i into the [p][n] tile.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lstm_bwd_gemm_f32_kernel(
    const float* __restrict__ dz, const float* __restrict__ flat, long k_off, float* __restrict__ dx, int lddx,
    float* __restrict__ dh_prev, int F, int H, int B) {
  __shared__ float Bs[2][32 * LF32_BSTR];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int grp = l >> 4, c16 = l & 15;
  const int row0 = blockIdx.x * 64 + w * 16;
  const int n0 = blockIdx.y * 64;
  const int G4 = 4 * H;
  const int arow = row0 + c16;
  const bool av = arow < B;
  const int sp = tid & 31, sn = tid >> 5;
  const float* Kg = flat + k_off + (long)(n0 + sn) * G4 + sp;
  float rb[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) rb[i] = Kg[(long)(8 * i) * G4];
  f4v acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = {0.f, 0.f, 0.f, 0.f};
  const int nsteps = G4 / 32;
  for (int st = 0; st < nsteps; ++st) {
    const int buf = st & 1, p0 = st * 32;
#pragma unroll
    for (int i = 0; i < 8; ++i) Bs[buf][sp * LF32_BSTR + sn + 8 * i] = rb[i];
    __syncthreads();
    if (st + 1 < nsteps) {
#pragma unroll
      for (int i = 0; i < 8; ++i) rb[i] = Kg[(long)(8 * i) * G4 + p0 + 32];
    }
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (av) ld8(dz + (long)arow * G4 + p0 + 8 * grp, v);
    mma_step(v, Bs[buf], grp, c16, acc);
  }
  if (row0 >= B) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + j * 16 + c16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + 4 * grp + r;
      if (row >= B) continue;
      if (n < F) dx[(long)row * lddx + n] = acc[j][r];
      else dh_prev[(long)row * H + (n - F)] = acc[j][r];
    }
  }
}

// ---------------------------------------------------------------------------
// weight gradient, partial slabs.  grid ((F+H)/64, 4H/64, nchunks): a workgroup owns dK[n0b:+64][p0b:+64] of chunk
// blockIdx.z's rows, walked 32 at a time in row order (csrc/trunk_f32.hip fc_wgrad_f32).  Xs / Gs rows of 64 fp32
// (+16 pad); D[n][p] += sum_rows xh[row][n] dz[row][p].  The blockIdx.x == 0 workgroups also write the chunk's db
// from fixed per-thread partials + an ordered LDS sum.  Slab of chunk c: part + c * (KK*G4 + G4), dK then db.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lstm_wgrad_f32_kernel(const float* __restrict__ xh,
                                                             const float* __restrict__ dz,
                                                             float* __restrict__ part, int F, int H, long R) {
  constexpr int S = 64 + 16;
  __shared__ __attribute__((aligned(16))) float Xs[32 * S];
  __shared__ __attribute__((aligned(16))) float Gs[32 * S];
  __shared__ float bred[32 * 64];
  const int KK = F + H, G4 = 4 * H;
  const int n0b = blockIdx.x * 64, p0b = blockIdx.y * 64;
  const long r_beg = (long)blockIdx.z * LF32_CHUNK;
  const long r_end = min(R, r_beg + LF32_CHUNK);
  float* slab = part + (long)blockIdx.z * ((long)KK * G4 + G4);
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int grp = l >> 4, i16 = l & 15;
  f4v acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a) { acc[a][0] = {0.f, 0.f, 0.f, 0.f}; acc[a][1] = {0.f, 0.f, 0.f, 0.f}; }
  float bpart[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int srow = tid >> 3, sc = (tid & 7) * 8;
  const int mt0 = 2 * (w >> 1), nt0 = 2 * (w & 1);
  for (long rb = r_beg; rb < r_end; rb += 32) {
    const long r = rb + srow;
    float xv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (r < r_end) {
      ld8(xh + r * KK + n0b + sc, xv);
      ld8(dz + r * G4 + p0b + sc, gv);
#pragma unroll
      for (int c = 0; c < 8; ++c) bpart[c] += gv[c];
    }
    st8(Xs + srow * S + sc, xv);
    st8(Gs + srow * S + sc, gv);
    __syncthreads();
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const int rr = 4 * jj + grp;
      float af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[i] = Xs[rr * S + (mt0 + i) * 16 + i16];
        bf[i] = Gs[rr * S + (nt0 + i) * 16 + i16];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jn = 0; jn < 2; ++jn)
          acc[i][jn] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[jn], acc[i][jn], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jn = 0; jn < 2; ++jn)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0b + (mt0 + i) * 16 + 4 * grp + r;
        const int p = p0b + (nt0 + jn) * 16 + i16;
        slab[(long)n * G4 + p] = acc[i][jn][r];
      }
  if (blockIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 8; ++c) bred[srow * 64 + sc + c] = bpart[c];
    __syncthreads();
    if (tid < 64) {
      float s = 0.f;
      for (int rr = 0; rr < 32; ++rr) s += bred[rr * 64 + tid];
      slab[(long)KK * G4 + p0b + tid] = s;
    }
  }
}

// grad[k_off + i] += sum_c slab_c.dK[i], grad[b_off + p] += sum_c slab_c.db[p], the slabs summed in chunk order
__global__ __launch_bounds__(256) void lstm_wgrad_reduce_f32_kernel(const float* __restrict__ part,
                                                                    float* __restrict__ grad, long k_off,
                                                                    long b_off, long n_k, int G4, int nchunks) {
  const long n_el = n_k + G4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_el; i += (long)gridDim.x * 256) {
    float s = 0.f;
    for (int c = 0; c < nchunks; ++c) s += part[(long)c * n_el + i];
    const long o = i < n_k ? k_off + i : b_off + (i - n_k);
    grad[o] += s;
  }
}

}  // namespace lstmf32
using namespace lstmf32;

extern "C" {

int launch_lstm_fwd_f32(const float* X, int ldx, const float* hprev, const float* cprev, const uint8_t* prev_done,
                        const float* flat, long k_off, long b_off, float* hout, float* cout, float* gates, float* xh,
                        int F, int H, int B, hipStream_t stream) {
  if (ldx <= 0 || F <= 0 || H <= 0 || B <= 0 || k_off < 0 || b_off < 0) return -22;
  if (F % 64 != 0 || H % 64 != 0 || ldx % 4 != 0 || ldx < F) return -1;
  dim3 grid((B + 63) / 64, H / 16);
  lstm_fwd_f32_kernel<<<grid, 256, 0, stream>>>(X, ldx, hprev, cprev, prev_done, flat, k_off, b_off, hout, cout,
                                                gates, xh, F, H, B);
  return (int)hipGetLastError();
}

int launch_lstm_bwd_gemm_f32(const float* dz, const float* flat, long k_off, float* dx, int lddx, float* dh_prev,
                             int F, int H, int B, hipStream_t stream) {
  if (lddx <= 0 || F <= 0 || H <= 0 || B <= 0 || k_off < 0) return -22;
  if (F % 64 != 0 || H % 64 != 0 || lddx < F) return -1;
  dim3 grid((B + 63) / 64, (F + H) / 64);
  lstm_bwd_gemm_f32_kernel<<<grid, 256, 0, stream>>>(dz, flat, k_off, dx, lddx, dh_prev, F, H, B);
  return (int)hipGetLastError();
}

// rows per partial slab of the weight gradient, and the scratch floats launch_lstm_wgrad_f32 needs for R rows
int lstm_wgrad_f32_chunk_rows() { return LF32_CHUNK; }
long lstm_wgrad_f32_part_numel(int F, int H, long R) {
  if (F <= 0 || H <= 0 || R <= 0) return 0;
  const long nch = (R + LF32_CHUNK - 1) / LF32_CHUNK;
  return nch * ((long)(F + H) * 4 * H + 4L * H);
}

int launch_lstm_wgrad_f32(const float* xh, const float* dz, float* grad, float* part, long k_off, long b_off, int F,
                          int H, long R, hipStream_t stream) {
  if (F <= 0 || H <= 0 || R <= 0 || k_off < 0 || b_off < 0 || !part) return -22;
  if (F % 64 != 0 || H % 64 != 0) return -1;
  const long nch = (R + LF32_CHUNK - 1) / LF32_CHUNK;
  if (nch > 65535) return -1;
  const int G4 = 4 * H;
  const long n_k = (long)(F + H) * G4;
  dim3 grid((F + H) / 64, G4 / 64, (unsigned)nch);
  lstm_wgrad_f32_kernel<<<grid, 256, 0, stream>>>(xh, dz, part, F, H, R);
  lstm_wgrad_reduce_f32_kernel<<<(unsigned)min((n_k + G4 + 255) / 256, 2048L), 256, 0, stream>>>(
      part, grad, k_off, b_off, n_k, G4, (int)nch);
  return (int)hipGetLastError();
}
}
