"""The float64 restatement of the PPO / A2C head loss (ppo/agent.py:96-137, a2c/agent.py:
190-218) that the GPU tests of the executor path and of xa_ac_head_grad compare with."""
import numpy as np
import oracle as OR

LOG2PI = np.log(2 * np.pi)


def heads_terms_f64(out_a, v, act, oldlp, oldv, ret, kind, dist='logits', clip=0.1,
                    ent_coef=0.01, v_coef=0.5, eps=1e-8):
    """Per-sample loss terms and d (mean loss) / d actor output, d / d value for
    MultivariateNormalDiag(loc = out_a) ('gauss') or a Categorical over softmax(out_a)
    ('logits', 'softmax'). TF tie rules: tf.maximum sends the gradient to its first input
    when x >= y, tf.clip_by_value passes it when lo <= x <= hi. For PPO the dict also
    holds what decides the branches (ratio, dvo, pg1, pg2, vl1, vl2)."""
    out_a, v, oldlp, oldv, ret = (np.asarray(x, np.float64) for x in (out_a, v, oldlp, oldv, ret))
    n = out_a.shape[0]
    if dist == 'gauss':
        d = out_a.shape[1]
        diff = np.asarray(act, np.float64) - out_a
        logp = -0.5 * (diff ** 2).sum(1) - 0.5 * d * LOG2PI
        dlogp_dz = diff
        H = np.full(n, 0.5 * d * (1 + LOG2PI))
        dH = np.zeros_like(out_a)
    else:
        a = np.asarray(act).astype(int)
        lsm = OR.log_softmax(out_a)
        p = np.exp(lsm)
        logp = lsm[np.arange(n), a]
        H = -(p * lsm).sum(-1)
        dlogp_dz = np.eye(out_a.shape[1])[a] - p
        dH = -p * (lsm + H[:, None])  # dH/dz
    t = dict(logp=logp, ent=H)
    if kind == 'ppo':
        adv = ret - oldv
        adv = (adv - adv.mean()) / (adv.std() + eps)
        ratio = np.exp(logp - oldlp)
        pg1, pg2 = -adv * ratio, -adv * np.clip(ratio, 1 - clip, 1 + clip)
        r_in = (ratio >= 1 - clip) & (ratio <= 1 + clip)
        dlogp = np.where((pg1 >= pg2) | r_in, -adv * ratio, 0.0) / n
        dvo = v - oldv
        vclip = oldv + np.clip(dvo, -clip, clip)
        vl1, vl2 = (v - ret) ** 2, (vclip - ret) ** 2
        v_in = (dvo >= -clip) & (dvo <= clip)
        dv = v_coef * 0.5 * np.where(vl1 >= vl2, 2 * (v - ret),
                                     np.where(v_in, 2 * (vclip - ret), 0.0)) / n
        t.update(pg=np.maximum(pg1, pg2), vl=np.maximum(vl1, vl2), ratio=ratio, dvo=dvo,
                 pg1=pg1, pg2=pg2, vl1=vl1, vl2=vl2, r_in=r_in, v_in=v_in)
    else:
        dlogp = -(ret - oldv) / n
        dv = v_coef * 2 * (v - ret) / n
        t.update(pg=-(ret - oldv) * logp, vl=(v - ret) ** 2)
    t.update(dz=dlogp[:, None] * dlogp_dz - (ent_coef / n) * dH, dv=dv)
    return t


def heads_f64(*args, **kw):
    """(d loss / d actor output, d loss / d value, log-prob of the actions)."""
    t = heads_terms_f64(*args, **kw)
    return t['dz'], t['dv'], t['logp']
