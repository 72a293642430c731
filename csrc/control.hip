// Classic-control vector environments on device (bit-identical resets, fp32 dynamics as envs/control.py and
// envs/cartpole.py): Acrobot-v1, MountainCar-v0 and CartPole-v1 with a padded observation row.
//
// One kernel template over the game, thread per env, 256 threads per workgroup, no LDS, no atomics; it follows
// cartpole_step_kernel (csrc/envs.hip).  state [B][NS] f32, steps [B] i32, epret [B] f32, counter [B] u32.
// The observation of the state AFTER the step (after the auto-reset where the episode ended) goes to either or
// both of
//   * obs_f32: fp32 rows of stride obs_ld floats (NO <= obs_ld <= 8), columns NO..obs_ld-1 written as zeros;
//   * obs_bf16: bf16 [B][8] rows, zero padded, one 16-byte store per env.
// Reset values are u * scale - offset with a separately rounded multiply and subtract (reset_val: no fused
// multiply-add), which is what torch computes, so both sides reset bit-equal.
#include "common.h"

namespace control {

constexpr float PI_F = 3.14159265358979323846f;

DEVI float reset_u(uint32_t seed, uint32_t env, uint32_t ctr, uint32_t s) {
  return (float)(env_rand_u32(seed, env, ctr, s) >> 8) * (1.0f / 16777216.0f);
}
// u * scale - off in two roundings: contraction is switched off for this body (hipcc contracts a * b - c into a fused
// multiply-add by default, through __fmul_rn / __fsub_rn as well, which are plain operators there); the operations
// keep that property when the function is inlined
DEVI float reset_val(float u, float scale, float off) {
#pragma clang fp contract(off)
  const float m = u * scale;
  return m - off;
}
DEVI float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// ---- CartPole-v1 (the dynamics of cartpole_step_kernel) ---------------------------------------------------------
struct CartPole {
  static constexpr int NS = 4, NO = 4;
  DEVI static void reset(float* s, uint32_t seed, uint32_t env, uint32_t ctr) {
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = reset_val(reset_u(seed, env, ctr, (uint32_t)i), 0.1f, 0.05f);
  }
  // -> terminal; reward of the step in r
  DEVI static bool step(float* s, int a, float& r) {
    const float g = 9.8f, mc = 1.0f, mp = 0.1f, tm = mc + mp, len = 0.5f, pml = mp * len, fm = 10.0f, tau = 0.02f;
    const float th_thr = 12.f * 2.f * PI_F / 360.f, x_thr = 2.4f;
    float x = s[0], xd = s[1], th = s[2], thd = s[3];
    const float force = a == 1 ? fm : -fm;
    const float ct = cosf(th), st = sinf(th);
    const float temp = (force + pml * thd * thd * st) / tm;
    const float thacc = (g * st - ct * temp) / (len * (4.0f / 3.0f - mp * ct * ct / tm));
    const float xacc = temp - pml * thacc * ct / tm;
    x = x + tau * xd;
    xd = xd + tau * xacc;
    th = th + tau * thd;
    thd = thd + tau * thacc;
    s[0] = x; s[1] = xd; s[2] = th; s[3] = thd;
    r = 1.0f;
    return x < -x_thr || x > x_thr || th < -th_thr || th > th_thr;
  }
  DEVI static void observe(const float* s, float* o) {
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = s[i];
  }
};

// ---- MountainCar-v0 ---------------------------------------------------------------------------------------------
struct MountainCar {
  static constexpr int NS = 2, NO = 2;
  DEVI static void reset(float* s, uint32_t seed, uint32_t env, uint32_t ctr) {
    s[0] = reset_val(reset_u(seed, env, ctr, 0u), 0.2f, 0.6f);
    s[1] = 0.f;
  }
  DEVI static bool step(float* s, int a, float& r) {
    if (a >= 3 || a < 0) a = 0;
    float p = s[0], v = s[1];
    v = v + ((float)(a - 1) * 0.001f + cosf(3.0f * p) * (-0.0025f));
    v = clampf(v, -0.07f, 0.07f);
    p = clampf(p + v, -1.2f, 0.6f);
    if (p == -1.2f && v < 0.f) v = 0.f;
    s[0] = p; s[1] = v;
    r = -1.0f;
    return p >= 0.5f && v >= 0.f;
  }
  DEVI static void observe(const float* s, float* o) { o[0] = s[0]; o[1] = s[1]; }
};

// ---- Acrobot-v1 ("book" dynamics, RK4, no torque noise) ---------------------------------------------------------
struct Acrobot {
  static constexpr int NS = 4, NO = 6;
  DEVI static void reset(float* s, uint32_t seed, uint32_t env, uint32_t ctr) {
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = reset_val(reset_u(seed, env, ctr, (uint32_t)i), 0.2f, 0.1f);
  }
  // d/dt (th1, th2, w1, w2) at torque tau; m1 = m2 = 1, l1 = 1, lc1 = lc2 = 0.5, I1 = I2 = 1, g = 9.8
  DEVI static void dsdt(const float* s, float tau, float* d) {
    const float m1 = 1.f, m2 = 1.f, l1 = 1.f, lc1 = 0.5f, lc2 = 0.5f, I1 = 1.f, I2 = 1.f, g = 9.8f;
    const float th1 = s[0], th2 = s[1], w1 = s[2], w2 = s[3];
    const float c2 = cosf(th2), s2 = sinf(th2);
    const float d1 = m1 * lc1 * lc1 + m2 * (l1 * l1 + lc2 * lc2 + 2.f * l1 * lc2 * c2) + I1 + I2;
    const float d2 = m2 * (lc2 * lc2 + l1 * lc2 * c2) + I2;
    const float phi2 = m2 * lc2 * g * cosf(th1 + th2 - PI_F / 2.f);
    const float phi1 = -m2 * l1 * lc2 * w2 * w2 * s2 - 2.f * m2 * l1 * lc2 * w2 * w1 * s2 +
                       (m1 * lc1 + m2 * l1) * g * cosf(th1 - PI_F / 2.f) + phi2;
    const float a2 =
        (tau + d2 / d1 * phi1 - m2 * l1 * lc2 * w1 * w1 * s2 - phi2) / (m2 * lc2 * lc2 + I2 - d2 * d2 / d1);
    const float a1 = -(d2 * a2 + phi1) / d1;
    d[0] = w1; d[1] = w2; d[2] = a1; d[3] = a2;
  }
  DEVI static float wrap(float x) {
#pragma unroll
    for (int i = 0; i < 3; ++i) x = x > PI_F ? x - 2.f * PI_F : x;
#pragma unroll
    for (int i = 0; i < 3; ++i) x = x < -PI_F ? x + 2.f * PI_F : x;
    return x;
  }
  DEVI static bool step(float* s, int a, float& r) {
    if (a >= 3 || a < 0) a = 0;
    const float tau = (float)(a - 1), dt = 0.2f;
    float k1[4], k2[4], k3[4], k4[4], y[4];
    dsdt(s, tau, k1);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = s[i] + (dt * 0.5f) * k1[i];
    dsdt(y, tau, k2);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = s[i] + (dt * 0.5f) * k2[i];
    dsdt(y, tau, k3);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = s[i] + dt * k3[i];
    dsdt(y, tau, k4);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = s[i] + (dt / 6.f) * (k1[i] + 2.f * k2[i] + 2.f * k3[i] + k4[i]);
    s[0] = wrap(y[0]);
    s[1] = wrap(y[1]);
    s[2] = clampf(y[2], -4.f * PI_F, 4.f * PI_F);
    s[3] = clampf(y[3], -9.f * PI_F, 9.f * PI_F);
    const bool term = -cosf(s[0]) - cosf(s[0] + s[1]) > 1.0f;
    r = term ? 0.f : -1.0f;
    return term;
  }
  DEVI static void observe(const float* s, float* o) {
    o[0] = cosf(s[0]); o[1] = sinf(s[0]); o[2] = cosf(s[1]); o[3] = sinf(s[1]); o[4] = s[2]; o[5] = s[3];
  }
};

// observation rows of env b from its state s: fp32 row of obs_ld floats and / or bf16 [8] row, zero padded
template <class G>
DEVI void write_obs(const float* s, int b, float* __restrict__ obs_f32, int obs_ld, bf16_t* __restrict__ obs_bf16) {
  float o[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = 0.f;
  G::observe(s, o);
  if (obs_f32) {
    float* row = obs_f32 + (long)b * obs_ld;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < obs_ld) row[i] = o[i];
  }
  if (obs_bf16) {
    uint4 q;
    q.x = pack2bf(o[0], o[1]);
    q.y = pack2bf(o[2], o[3]);
    q.z = pack2bf(o[4], o[5]);
    q.w = pack2bf(o[6], o[7]);
    *reinterpret_cast<uint4*>(obs_bf16 + (long)b * 8) = q;
  }
}

template <class G>
__global__ void __launch_bounds__(256)
step_kernel(float* __restrict__ state, int* __restrict__ steps, float* __restrict__ epret,
            uint32_t* __restrict__ counter, const int* __restrict__ actions, int B, uint32_t seed, uint32_t id_base,
            int max_steps, float* __restrict__ obs_f32, int obs_ld, bf16_t* __restrict__ obs_bf16,
            float* __restrict__ reward_out, uint8_t* __restrict__ done_out, float* __restrict__ epret_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float s[G::NS];
#pragma unroll
  for (int i = 0; i < G::NS; ++i) s[i] = state[(long)b * G::NS + i];
  float r;
  const bool term = G::step(s, actions[b], r);
  const int n = steps[b] + 1;
  const bool done = term || n >= max_steps;
  const float er = epret[b] + r;
  uint32_t ctr = counter[b];
  reward_out[b] = r;
  done_out[b] = done;
  epret_out[b] = done ? er : 0.f;
  if (done) {
    G::reset(s, seed, id_base + (uint32_t)b, ctr);
    ctr += 1;
  }
  counter[b] = ctr;
  steps[b] = done ? 0 : n;
  epret[b] = done ? 0.f : er;
#pragma unroll
  for (int i = 0; i < G::NS; ++i) state[(long)b * G::NS + i] = s[i];
  write_obs<G>(s, b, obs_f32, obs_ld, obs_bf16);
}

// the observation of the state as it stands (no step): what the step kernel writes after its step, so an engine that
// starts or resumes from a stored state reads exactly the rows a rollout would have handed it
template <class G>
__global__ void __launch_bounds__(256)
observe_kernel(const float* __restrict__ state, int B, float* __restrict__ obs_f32, int obs_ld,
               bf16_t* __restrict__ obs_bf16) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float s[G::NS];
#pragma unroll
  for (int i = 0; i < G::NS; ++i) s[i] = state[(long)b * G::NS + i];
  write_obs<G>(s, b, obs_f32, obs_ld, obs_bf16);
}

template <class G>
int launch_observe(const float* state, int B, float* obs_f32, int obs_ld, void* obs_bf16, hipStream_t stream) {
  if (B <= 0 || obs_ld < G::NO || obs_ld > 8 || !state) return -22;
  observe_kernel<G><<<(B + 255) / 256, 256, 0, stream>>>(state, B, obs_f32, obs_ld, (bf16_t*)obs_bf16);
  return (int)hipGetLastError();
}

template <class G>
int launch(float* state, int* steps, float* epret, void* counter, const int* actions, int B, unsigned seed,
           unsigned id_base, int max_steps, float* obs_f32, int obs_ld, void* obs_bf16, float* reward, void* done,
           float* epret_out, hipStream_t stream) {
  if (B <= 0 || max_steps < 0 || obs_ld < G::NO || obs_ld > 8) return -22;
  if (!state || !steps || !epret || !counter || !actions || !reward || !done || !epret_out) return -22;
  step_kernel<G><<<(B + 255) / 256, 256, 0, stream>>>(state, steps, epret, (uint32_t*)counter, actions, B, seed,
                                                      id_base, max_steps, obs_f32, obs_ld, (bf16_t*)obs_bf16, reward,
                                                      (uint8_t*)done, epret_out);
  return (int)hipGetLastError();
}

}  // namespace control

extern "C" {
// obs_f32 (rows of obs_ld floats, native width <= obs_ld <= 8) and obs_bf16 ([B][8]) may each be null
int launch_acrobot_step(float* state, int* steps, float* epret, void* counter, const int* actions, int B,
                        unsigned seed, unsigned id_base, int max_steps, float* obs_f32, int obs_ld, void* obs_bf16,
                        float* reward, void* done, float* epret_out, hipStream_t stream) {
  return control::launch<control::Acrobot>(state, steps, epret, counter, actions, B, seed, id_base, max_steps, obs_f32,
                                           obs_ld, obs_bf16, reward, done, epret_out, stream);
}

int launch_mountaincar_step(float* state, int* steps, float* epret, void* counter, const int* actions, int B,
                            unsigned seed, unsigned id_base, int max_steps, float* obs_f32, int obs_ld, void* obs_bf16,
                            float* reward, void* done, float* epret_out, hipStream_t stream) {
  return control::launch<control::MountainCar>(state, steps, epret, counter, actions, B, seed, id_base, max_steps,
                                               obs_f32, obs_ld, obs_bf16, reward, done, epret_out, stream);
}

int launch_cartpole_step_padded(float* state, int* steps, float* epret, void* counter, const int* actions, int B,
                                unsigned seed, unsigned id_base, int max_steps, float* obs_f32, int obs_ld,
                                void* obs_bf16, float* reward, void* done, float* epret_out, hipStream_t stream) {
  return control::launch<control::CartPole>(state, steps, epret, counter, actions, B, seed, id_base, max_steps, obs_f32,
                                            obs_ld, obs_bf16, reward, done, epret_out, stream);
}

// game: 0 CartPole-v1, 1 Acrobot-v1, 2 MountainCar-v0; writes the observation rows of the stored states
int launch_control_observe(int game, const float* state, int B, float* obs_f32, int obs_ld, void* obs_bf16,
                           hipStream_t stream) {
  if (game == 0) return control::launch_observe<control::CartPole>(state, B, obs_f32, obs_ld, obs_bf16, stream);
  if (game == 1) return control::launch_observe<control::Acrobot>(state, B, obs_f32, obs_ld, obs_bf16, stream);
  if (game == 2) return control::launch_observe<control::MountainCar>(state, B, obs_f32, obs_ld, obs_bf16, stream);
  return -22;
}
}
