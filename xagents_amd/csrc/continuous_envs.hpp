// gym's two classic continuous-control ids on device: Pendulum-v1 and
// MountainCarContinuous-v0 step, reset and observation functions for the step kernel
// (continuous_envs.hip, one thread per env). Replaces gym's env.step / env.reset inside
// BaseAgent.step_envs (xagents/base.py:388-426, the gym call at base.py:408) for the two ids.
//
// As in classic_envs.hpp: state and arithmetic are f64, observations and rewards the f32
// rounding of the f64 values, every expression is written in one fixed order (the library is
// compiled with -ffp-contract=off) and the trigonometry is the device library's f64 sin / cos.
// gym itself is not part of this build: the formulas below are the project's statement of
// classic_control/pendulum.py and continuous_mountain_car.py.
#pragma once
#include "../../include/xagents_hip.h"
#include "classic_envs.hpp"  // kXaPi, xa_reset_uniforms

// ---- Pendulum-v1: state (th, thdot); g = 10, m = 1, l = 1, dt = 0.05, max_speed = 8,
// max_torque = 2. The env never terminates, TimeLimit 200. th is not wrapped in the state.
// Python's x % y for floats (floor modulo): fmod, moved into [0, y) for y > 0
XA_DEV double xa_fmod_floor(double x, double y) {
  double r = fmod(x, y);
  if (r != 0.0 && ((r < 0.0) != (y < 0.0))) r = r + y;
  return r;
}

// gym's angle_normalize: ((x + pi) % (2 pi)) - pi
XA_DEV double xa_pendulum_norm(double x) { return xa_fmod_floor(x + kXaPi, 2.0 * kXaPi) - kXaPi; }

// one step with the raw action; returns the reward -cost (cost from the pre-step state)
XA_DEV double xa_pendulum_step(double (&s)[2], double action) {
  const double g = 10.0, m = 1.0, l = 1.0, dt = 0.05, max_speed = 8.0, max_torque = 2.0;
  const double th = s[0], thdot = s[1];
  const double u = fmin(fmax(action, -max_torque), max_torque);
  const double nth = xa_pendulum_norm(th);
  const double cost = nth * nth + 0.1 * (thdot * thdot) + 0.001 * (u * u);
  double nthdot = thdot + (3.0 * g / (2.0 * l) * sin(th) + 3.0 / (m * (l * l)) * u) * dt;
  nthdot = fmin(fmax(nthdot, -max_speed), max_speed);  // the clip comes before the angle update
  s[0] = th + nthdot * dt;
  s[1] = nthdot;
  return -cost;
}

XA_DEV void xa_pendulum_reset(double (&s)[2], const double (&u)[4]) {
  s[0] = -kXaPi + 2.0 * kXaPi * u[0];
  s[1] = -1.0 + 2.0 * u[1];
}

XA_DEV void xa_pendulum_obs(const double (&s)[2], float (&o)[3]) {
  double sn, cs;
  sincos(s[0], &sn, &cs);
  o[0] = (float)cs;
  o[1] = (float)sn;
  o[2] = (float)s[1];
}

// ---- MountainCarContinuous-v0: state (x, v); power = 0.0015, max_speed = 0.07,
// x in [-1.2, 0.6], goal x >= 0.45 with v >= 0. TimeLimit 999. The reward's action penalty
// uses the raw action, not the clipped force.
XA_DEV bool xa_mountaincar_cont_step(double (&s)[2], double action, double& reward) {
  double x = s[0], v = s[1];
  const double f = fmin(fmax(action, -1.0), 1.0);
  v = v + (f * 0.0015 - 0.0025 * cos(3.0 * x));
  v = fmin(fmax(v, -0.07), 0.07);
  x = x + v;
  x = fmin(fmax(x, -1.2), 0.6);
  if (x == -1.2 && v < 0.0) v = 0.0;
  s[0] = x;
  s[1] = v;
  const bool terminated = x >= 0.45 && v >= 0.0;
  reward = (terminated ? 100.0 : 0.0) - 0.1 * (action * action);
  return terminated;
}

XA_DEV void xa_mountaincar_cont_reset(double (&s)[2], const double (&u)[4]) {
  s[0] = -0.6 + 0.2 * u[0];
  s[1] = 0.0;
}

XA_DEV void xa_mountaincar_cont_obs(const double (&s)[2], float (&o)[2]) {
  o[0] = (float)s[0];
  o[1] = (float)s[1];
}

// One interface over the two ids (KIND = XA_ENV_PENDULUM / XA_ENV_MOUNTAINCAR_CONT): the
// observation count, env.step with the raw action (returns gym's `terminated` and the f64
// reward; the caller adds the TimeLimit), env.reset from four uniforms, the observation.
template <int KIND>
struct XaContinuousEnv;

template <>
struct XaContinuousEnv<XA_ENV_PENDULUM> {
  static constexpr int kObs = 3;
  static XA_DEV bool step(double (&s)[2], double action, double& reward) {
    reward = xa_pendulum_step(s, action);
    return false;
  }
  static XA_DEV void reset(double (&s)[2], const double (&u)[4]) { xa_pendulum_reset(s, u); }
  static XA_DEV void obs(const double (&s)[2], float (&o)[3]) { xa_pendulum_obs(s, o); }
};

template <>
struct XaContinuousEnv<XA_ENV_MOUNTAINCAR_CONT> {
  static constexpr int kObs = 2;
  static XA_DEV bool step(double (&s)[2], double action, double& reward) {
    return xa_mountaincar_cont_step(s, action, reward);
  }
  static XA_DEV void reset(double (&s)[2], const double (&u)[4]) {
    xa_mountaincar_cont_reset(s, u);
  }
  static XA_DEV void obs(const double (&s)[2], float (&o)[2]) { xa_mountaincar_cont_obs(s, o); }
};
