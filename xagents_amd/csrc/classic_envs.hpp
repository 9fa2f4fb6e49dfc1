// gym classic-control dynamics on device: CartPole-v1, Acrobot-v1 and MountainCar-v0 step,
// reset and observation functions. All three run in the fused rollout (mlp_rollout.hip, one
// wave per env, wave-uniform); Acrobot and MountainCar also in the step kernel
// (classic_envs.hip, one thread per env). Replaces gym's env.step / env.reset inside
// BaseAgent.step_envs (xagents/base.py:388-426, the gym call at base.py:408) for the ids.
//
// State and arithmetic are f64, observations the f32 rounding of the f64 values. Every
// expression is written in one fixed order (the library is compiled with -ffp-contract=off;
// the only fused multiply-adds are the explicit fma calls of CartPole's small-angle
// polynomial) and the trigonometry is otherwise the device library's f64 sin / cos / sincos,
// so both kernels produce the same bits from the same state and action. The RK4 stages of
// Acrobot leave [-pi, pi] (|theta| up to ~9 rad), so CartPole's polynomial does not apply.
#pragma once
#include "../../include/xagents_hip.h"
#include "xa_common.hpp"

constexpr double kXaPi = 3.141592653589793;

// The uniforms of a reset at rollout step t of env: Philox keyed as the CartPole reset
// (env, step index, counter lo, counter hi ^ 0x5eed5eed; seed), u_k = word_k 2^-32.
XA_DEV void xa_reset_uniforms(int env, int t, uint64_t ctr, uint64_t seed, double (&u)[4]) {
  const xa_u4 rr = xa_philox((uint32_t)env, (uint32_t)t, (uint32_t)ctr,
                             (uint32_t)(ctr >> 32) ^ 0x5eed5eedu, (uint32_t)seed,
                             (uint32_t)(seed >> 32));
  const uint32_t rv[4] = {rr.x, rr.y, rr.z, rr.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) u[k] = (double)rv[k] * 2.3283064365386963e-10;
}

// ---- CartPole-v1 (classic_control/cartpole.py): state (x, x_dot, theta, theta_dot), Euler
// integration. Reward 1 every step, TimeLimit 500.
// sin and cos of a pole angle: |x| <= 0.5 rad (always, below the 0.2095-rad termination
// threshold plus one Euler step) by their Taylor series to x^15 / x^16 in Horner form on the
// f64 FMA unit (truncation < 2.3e-17, within an ulp of libm, like any two libms), larger
// angles by the library functions. The library sin / cos carry a branch-free Payne-Hanek
// reduction (~250 f64 instructions) that dominated the per-step dependency chain of the
// dynamics rollout.
XA_DEV void pole_sincos(double x, double& sn, double& cs) {
  if (fabs(x) > 0.5) {
    sn = sin(x);
    cs = cos(x);
    return;
  }
  const double x2 = x * x;
  double ps = 1.0 / 1307674368000.0;               // 1 / 15!
  ps = fma(ps, -x2, 1.0 / 6227020800.0);           // 1 / 13!
  ps = fma(ps, -x2, 1.0 / 39916800.0);             // 1 / 11!
  ps = fma(ps, -x2, 1.0 / 362880.0);               // 1 / 9!
  ps = fma(ps, -x2, 1.0 / 5040.0);                 // 1 / 7!
  ps = fma(ps, -x2, 1.0 / 120.0);                  // 1 / 5!
  ps = fma(ps, -x2, 1.0 / 6.0);                    // 1 / 3!
  sn = fma(-x * x2, ps, x);
  double pc = 1.0 / 20922789888000.0;              // 1 / 16!
  pc = fma(pc, -x2, 1.0 / 87178291200.0);          // 1 / 14!
  pc = fma(pc, -x2, 1.0 / 479001600.0);            // 1 / 12!
  pc = fma(pc, -x2, 1.0 / 3628800.0);              // 1 / 10!
  pc = fma(pc, -x2, 1.0 / 40320.0);                // 1 / 8!
  pc = fma(pc, -x2, 1.0 / 720.0);                  // 1 / 6!
  pc = fma(pc, -x2, 1.0 / 24.0);                   // 1 / 4!
  pc = fma(pc, -x2, 0.5);                          // 1 / 2!
  cs = fma(-x2, pc, 1.0);
}

XA_DEV bool cartpole_step(double (&s)[4], int action) {
  const double gravity = 9.8, masspole = 0.1, total_mass = 1.1, length = 0.5;
  const double polemass_length = 0.05, force_mag = 10.0, tau = 0.02;
  const double force = action == 1 ? force_mag : -force_mag;
  double sintheta, costheta;
  pole_sincos(s[2], sintheta, costheta);
  const double temp = (force + polemass_length * s[3] * s[3] * sintheta) / total_mass;
  const double thetaacc = (gravity * sintheta - costheta * temp) /
                          (length * (4.0 / 3.0 - masspole * costheta * costheta / total_mass));
  const double xacc = temp - polemass_length * thetaacc * costheta / total_mass;
  s[0] = s[0] + tau * s[1];
  s[1] = s[1] + tau * xacc;
  s[2] = s[2] + tau * s[3];
  s[3] = s[3] + tau * thetaacc;
  const double theta_thr = 12.0 * 2.0 * 3.141592653589793 / 360.0;
  return s[0] < -2.4 || s[0] > 2.4 || s[2] < -theta_thr || s[2] > theta_thr;
}

// ---- MountainCar-v0 (classic_control/mountain_car.py): state (position, velocity) in
// s[0], s[1]; s[2], s[3] are not touched. Reward -1 every step, TimeLimit 200.
XA_DEV bool xa_mountaincar_step(double (&s)[4], int action) {
  double p = s[0], v = s[1];
  v = v + ((double)(action - 1) * 0.001 + cos(3.0 * p) * (-0.0025));
  v = fmin(fmax(v, -0.07), 0.07);
  p = p + v;
  p = fmin(fmax(p, -1.2), 0.6);
  if (p == -1.2 && v < 0.0) v = 0.0;
  s[0] = p;
  s[1] = v;
  return p >= 0.5 && v >= 0.0;
}

XA_DEV void xa_mountaincar_reset(double (&s)[4], const double (&u)[4]) {
  s[0] = -0.6 + 0.2 * u[0];
  s[1] = 0.0;
}

XA_DEV void xa_mountaincar_obs(const double (&s)[4], float (&o)[2]) {
  o[0] = (float)s[0];
  o[1] = (float)s[1];
}

// ---- Acrobot-v1 (classic_control/acrobot.py), the "book" dynamics: m1 = m2 = 1, l1 = 1,
// lc1 = lc2 = 0.5, I1 = I2 = 1, g = 9.8, dt = 0.2, no torque noise. State (theta1, theta2,
// dtheta1, dtheta2). Reward -1, 0 on the terminal step, TimeLimit 500.
XA_DEV void xa_acrobot_dsdt(const double (&s)[4], double tau, double (&ds)[4]) {
  const double m1 = 1.0, m2 = 1.0, l1 = 1.0, lc1 = 0.5, lc2 = 0.5, I1 = 1.0, I2 = 1.0, g = 9.8;
  const double th1 = s[0], th2 = s[1], w1 = s[2], w2 = s[3];
  double sn2, cs2;
  sincos(th2, &sn2, &cs2);
  const double d1 = m1 * (lc1 * lc1) + m2 * (l1 * l1 + lc2 * lc2 + 2.0 * l1 * lc2 * cs2) + I1 + I2;
  const double d2 = m2 * (lc2 * lc2 + l1 * lc2 * cs2) + I2;
  const double phi2 = m2 * lc2 * g * cos(th1 + th2 - kXaPi / 2.0);
  const double phi1 = -m2 * l1 * lc2 * (w2 * w2) * sn2 - 2.0 * m2 * l1 * lc2 * w2 * w1 * sn2 +
                      (m1 * lc1 + m2 * l1) * g * cos(th1 - kXaPi / 2.0) + phi2;
  const double dd2 = (tau + d2 / d1 * phi1 - m2 * l1 * lc2 * (w1 * w1) * sn2 - phi2) /
                     (m2 * (lc2 * lc2) + I2 - d2 * d2 / d1);
  const double dd1 = -(d2 * dd2 + phi1) / d1;
  ds[0] = w1;
  ds[1] = w2;
  ds[2] = dd1;
  ds[3] = dd2;
}

// gym's wrap(): repeated -+ 2 pi into [-pi, pi]. With both velocities clipped an RK4 step
// moves an angle by well under 64 turns, so the loops are bounded there: a state that is not
// an Acrobot state (infinite, uninitialised memory) cannot hang the kernel.
XA_DEV double xa_acrobot_wrap(double x) {
  const double diff = kXaPi - (-kXaPi);
  for (int i = 0; i < 64 && x > kXaPi; ++i) x = x - diff;
  for (int i = 0; i < 64 && x < -kXaPi; ++i) x = x + diff;
  return x;
}

XA_DEV bool xa_acrobot_step(double (&s)[4], int action) {
  const double tau = (double)(action - 1);
  const double dt = 0.2, dt2 = 0.1;
  double k1[4], k2[4], k3[4], k4[4], y[4];
  xa_acrobot_dsdt(s, tau, k1);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = s[i] + dt2 * k1[i];
  xa_acrobot_dsdt(y, tau, k2);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = s[i] + dt2 * k2[i];
  xa_acrobot_dsdt(y, tau, k3);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = s[i] + dt * k3[i];
  xa_acrobot_dsdt(y, tau, k4);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    y[i] = s[i] + dt / 6.0 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
  s[0] = xa_acrobot_wrap(y[0]);
  s[1] = xa_acrobot_wrap(y[1]);
  s[2] = fmin(fmax(y[2], -4.0 * kXaPi), 4.0 * kXaPi);
  s[3] = fmin(fmax(y[3], -9.0 * kXaPi), 9.0 * kXaPi);
  return -cos(s[0]) - cos(s[1] + s[0]) > 1.0;
}

XA_DEV void xa_acrobot_reset(double (&s)[4], const double (&u)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = -0.1 + 0.2 * u[k];
}

XA_DEV void xa_acrobot_obs(const double (&s)[4], float (&o)[6]) {
  double sn1, cs1, sn2, cs2;
  sincos(s[0], &sn1, &cs1);
  sincos(s[1], &sn2, &cs2);
  o[0] = (float)cs1;
  o[1] = (float)sn1;
  o[2] = (float)cs2;
  o[3] = (float)sn2;
  o[4] = (float)s[2];
  o[5] = (float)s[3];
}

// One interface over the ids (KIND = XA_ENV_CARTPOLE / XA_ENV_ACROBOT / XA_ENV_MOUNTAINCAR;
// xa_classic_step takes the last two): observation and action counts, env.step (returns
// gym's `terminated`; the caller adds the TimeLimit), the step's reward, env.reset from four
// uniforms, the observation.
template <int KIND>
struct XaClassicEnv;

template <>
struct XaClassicEnv<XA_ENV_CARTPOLE> {
  static constexpr int kObs = 4, kActions = 2;
  static XA_DEV bool step(double (&s)[4], int action) { return cartpole_step(s, action); }
  static XA_DEV float reward(bool) { return 1.0f; }
  // np_random.uniform(-0.05, 0.05, size=(4,))
  static XA_DEV void reset(double (&s)[4], const double (&u)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = -0.05 + 0.1 * u[k];
  }
  static XA_DEV void obs(const double (&s)[4], float (&o)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (float)s[k];
  }
};

template <>
struct XaClassicEnv<XA_ENV_ACROBOT> {
  static constexpr int kObs = 6, kActions = 3;
  static XA_DEV bool step(double (&s)[4], int action) { return xa_acrobot_step(s, action); }
  static XA_DEV float reward(bool terminated) { return terminated ? 0.0f : -1.0f; }
  static XA_DEV void reset(double (&s)[4], const double (&u)[4]) { xa_acrobot_reset(s, u); }
  static XA_DEV void obs(const double (&s)[4], float (&o)[6]) { xa_acrobot_obs(s, o); }
};

template <>
struct XaClassicEnv<XA_ENV_MOUNTAINCAR> {
  static constexpr int kObs = 2, kActions = 3;
  static XA_DEV bool step(double (&s)[4], int action) { return xa_mountaincar_step(s, action); }
  static XA_DEV float reward(bool) { return -1.0f; }
  static XA_DEV void reset(double (&s)[4], const double (&u)[4]) { xa_mountaincar_reset(s, u); }
  static XA_DEV void obs(const double (&s)[4], float (&o)[2]) { xa_mountaincar_obs(s, o); }
};
