"""The search self-play rules of include/hexgnn.h (hexgnn_search_root_noise, hexgnn_search_record, hexgnn_samples_finish,
hexgnn_pv_loss) restated on the host (shared by tests/test_search_selfplay_host.py and tests/test_gpu_search_selfplay.py).
Written from the rules; shares no code with the kernels.

What is exact and what is not.  The visit distribution is one fp32 division of two integers below 2^24: bit-comparable.  The
proportional pick is integer arithmetic: exact.  The root's mean value and the sums of the loss are fp32 sums in an order the
header fixes; the oracle computes them in float64 and the tests bound the difference.  The root noise is a handful of fp32
operations behind one fp32 sum of at most hex_size^2 non-negative terms: relative 1e-6 covers it with room (the sum's
relative error is at most 7 x 2^-24 = 4e-7 for the 6 levels of a 64-lane scan plus the carries of up to 10 chunks, each of the
five further operations adds 2^-24 = 6e-8, and every term is non-negative: no cancellation)."""
import numpy as np

from search_oracle import first_max


def root_noise64(P, noise, eps):
    """(1 - eps) P + eps noise / sum(noise) over a root's edges, float64; None when the rule refuses the noise."""
    noise = np.asarray(noise, dtype=np.float64)
    S = noise.sum()
    if not np.isfinite(noise).all() or (noise < 0).any() or not (S > 0 and np.isfinite(S)):
        return None
    return (1.0 - float(eps)) * np.asarray(P, dtype=np.float64) + float(eps) * (noise / S)


def visit_policy(moves, N, cells):
    """policy row: N / T on the cells of the root's moves, zeros elsewhere; fp32, one division per edge."""
    N = np.asarray(N, dtype=np.int64)
    T = int(N.sum())
    row = np.zeros(cells, dtype=np.float32)
    row[np.asarray(moves, dtype=np.int64) - 2] = N.astype(np.float32) / np.float32(T)
    return row


def prop_k(u, T):
    """The integer the proportional pick compares the running sums with."""
    t = int(np.float32(u) * np.float32(16777216.0))
    assert 0 <= t < 1 << 24
    return (t * int(T)) >> 24


def proportional_pick(N, u):
    """Edge index: the first edge whose inclusive running sum of N exceeds k."""
    run, k = 0, prop_k(u, int(np.sum(N)))
    for e, n in enumerate(N):
        run += int(n)
        if run > k:
            return e
    raise AssertionError("k = %d is not below T = %d" % (k, run))


def greedy_pick(N):
    return first_max(np.asarray(N, dtype=np.float64))


def z_label(winner, side):
    """+1 when the side to move at the sample (side 1 = maker) won the game (winner 0 = maker), else -1; NaN undecided."""
    if winner < 0:
        return np.float32(np.nan)
    return np.float32(1.0 if (winner == 0) == (side == 1) else -1.0)


def sign(x):
    return (x > 0) - (x < 0)


def pv_loss(logp, target, value, z, root_q, q_ratio, val_factor, pol_factor, dtype=np.float64):
    """``logp`` / ``target``: per graph the log-policy rows and the targets on the same rows.  Returns ``(loss, per_graph [b, 4],
    d_logp (concatenated), d_value [b])`` in ``dtype``; the two hit columns are exact in any dtype."""
    f = dtype
    b = len(logp)
    per = np.zeros((b, 4), dtype=f)
    d_logp, d_value = [], np.zeros(b, dtype=f)
    q_ratio, val_factor, pol_factor = f(q_ratio), f(val_factor), f(pol_factor)
    for g in range(b):
        lp, t = np.asarray(logp[g], dtype=f), np.asarray(target[g], dtype=f)
        y = (f(1) - q_ratio) * f(z[g]) + q_ratio * f(root_q[g])
        d = f(value[g]) - y
        per[g, 0] = (-t * lp).sum(dtype=f)
        per[g, 1] = d * d
        per[g, 2] = float(len(lp) > 0 and first_max(np.asarray(logp[g])) == first_max(np.asarray(target[g])))
        per[g, 3] = float(sign(float(value[g])) == sign(float(y)))
        d_logp.append(-pol_factor * t)
        d_value[g] = f(2) * val_factor * d
    loss = val_factor * per[:, 1].sum(dtype=f) + pol_factor * per[:, 0].sum(dtype=f)
    return loss, per, (np.concatenate(d_logp) if d_logp else np.zeros(0, f)), d_value
