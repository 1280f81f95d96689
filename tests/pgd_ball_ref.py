"""float64 / integer statement of the PGD threat-model kernels (csrc/pgd_ball.hip, include/rmcl.h "PGD threat models"), in numpy.

Every function works on the values the kernel READS: lr, eps, lo, hi are rounded to fp32 first (the ABI carries floats), gradients are
widened from their storage type.  Each returns the float64 result and a per-element allowance for the fp32 kernel, derived the way
``pgd_reference`` of tests/test_step_kernels_gpu.py derives its own, with u = 2^-24 (one fp32 rounding, relative):

  step  = lr * num / den      product, quotient, and den itself (the fp32 rounding of a double-accumulated norm; the double sum of n
                              squares adds at most n 2^-53 relative, below 1e-10 u at n = 442 368): 3 u |step|
  t     = delta0 + step       one more rounding, u |t| <= u (|delta0| + |step|)
                              -> allowed_t = 4 u (|delta0| + |step|)          (the existing PGD allowance)
  L-inf clamp                 exact
  L2 scale t' = t * s         s = eps / fp32(||t||): two roundings, the product a third: 3 u |t'|; the norm is taken over the kernel's
                              own t, whose distance from the exact t is at most ||allowed_t||_2, i.e. rel_n = ||allowed_t||_2 / ||t||_2
                              -> allowed_t' = allowed_t + (3 u + rel_n) |t'|   (also covers a sample on the edge of the ball)
  no box   delta = t'                                  allowed_t'
           x = base + t'                               allowed_t' + u |x|
  box      x = clamp(base + t', lo, hi)                allowed_t' + u |base + t'|     (the clamp is 1-Lipschitz)
           delta = x - base                            allowed_x + u |delta|
  operand in bf16                                      + 2^-8 |x|: half a bf16 ulp (8 significand bits) of the value being cast
Pad slots (index >= valid[b]) are exact: delta = 0, operand = cast(base)."""
import numpy as np

U = 2.0 ** -24
DIR_NORMALISED, DIR_SIGN, DIR_L2 = 0, 1, 2
BALL_LINF, BALL_L2 = 0, 1


def f32(v):
    return float(np.float32(v))


def rng_hash(seed, idx):
    """rmcl_rng_hash of csrc/rmcl_common.h on numpy uint32 (wrapping arithmetic), elementwise over idx."""
    with np.errstate(over="ignore"):
        x = np.asarray(idx, dtype=np.uint32) * np.uint32(0x9E3779B1) ^ np.uint32(seed)
        x ^= x >> np.uint32(16)
        x = x * np.uint32(0x85EBCA6B)
        x ^= x >> np.uint32(13)
        x = x * np.uint32(0xC2B2AE35)
        x ^= x >> np.uint32(16)
    return x


def start_draw(seed, sample, n):
    """v = 2u - 1 with u = (h >> 8) 2^-24, h = hash(hash(seed, sample), i), i < n: float64 values that fp32 holds exactly."""
    ss = rng_hash(seed, np.uint32(sample))
    h = rng_hash(ss, np.arange(n, dtype=np.uint32))
    return (h >> np.uint32(8)).astype(np.float64) * 2.0 ** -23 - 1.0


def valid_mask(valid, B, per):
    m = np.ones((B, per), dtype=bool)
    if valid is not None:
        m = np.arange(per)[None, :] < np.clip(np.asarray(valid, dtype=np.int64), 0, per)[:, None]
    return m


def _finish(tp, allowed_tp, base, mask, box, bf16_operand):
    """box and operand of a projected step tp (0 on pads): (delta, allowed_delta, x, allowed_x)"""
    if base is None:
        return tp, allowed_tp, None, None
    raw = base + tp
    if box is not None:
        lo, hi = f32(box[0]), f32(box[1])
        x = np.where(mask, np.clip(raw, lo, hi), base)
        allowed_x = np.where(mask, allowed_tp + U * np.abs(raw), 0.0)
        delta = np.where(mask, x - base, 0.0)
        allowed_d = np.where(mask, allowed_x + U * np.abs(delta), 0.0)
    else:
        x = np.where(mask, raw, base)
        allowed_x = np.where(mask, allowed_tp + U * np.abs(raw), 0.0)
        delta, allowed_d = tp, allowed_tp
    if bf16_operand:
        allowed_x = np.where(mask, allowed_x * (1 + 2.0 ** -8) + 2.0 ** -8 * np.abs(x), 2.0 ** -8 * np.abs(x))
    return delta, allowed_d, x, allowed_x


def step_ball(g, delta0, lr, eps, direction, ball, base=None, box=None, valid=None, delta_zero=False, bf16_operand=False):
    """One rmcl_pgd_step_ball call.  g, delta0, base: [B, per] arrays (any float type).  Returns a dict: delta, allowed_delta, x (the
    operand before its cast), allowed_x, t (the unprojected step), scale [B] (L2 ball), raw (base + t' before the box)."""
    g = np.asarray(g, dtype=np.float64)
    B, per = g.shape
    mask = valid_mask(valid, B, per)
    lr, eps = f32(lr), f32(eps)
    d0 = np.zeros_like(g) if delta_zero else np.asarray(delta0, dtype=np.float64)
    gm = np.where(mask, g, 0.0)
    if direction == DIR_NORMALISED:
        den = np.maximum(np.abs(gm).max(axis=1, keepdims=True, initial=0.0), f32(1e-8))
        num = g
    elif direction == DIR_SIGN:
        den, num = np.ones((B, 1)), np.sign(g)
    elif direction == DIR_L2:
        den = np.maximum(np.sqrt((gm * gm).sum(axis=1, keepdims=True)), f32(1e-12))
        num = g
    else:
        raise ValueError(direction)
    step = np.where(mask, lr * num / den, 0.0)
    t = np.where(mask, d0 + step, 0.0)
    allowed_t = np.where(mask, 4 * U * (np.abs(d0) + np.abs(step)), 0.0)
    scale = np.ones(B)
    if eps > 0 and ball == BALL_LINF:
        tp, allowed_tp = np.clip(t, -eps, eps), allowed_t
    elif eps > 0 and ball == BALL_L2:
        nrm = np.sqrt((t * t).sum(axis=1))
        scale = np.where(nrm > eps, eps / np.maximum(nrm, 1e-300), 1.0)
        tp = t * scale[:, None]
        rel_n = np.sqrt((allowed_t ** 2).sum(axis=1)) / np.maximum(nrm, 1e-300)
        allowed_tp = allowed_t + (3 * U + rel_n)[:, None] * np.abs(tp)
    elif ball in (BALL_LINF, BALL_L2):
        tp, allowed_tp = t, allowed_t
    else:
        raise ValueError(ball)
    base64 = None if base is None else np.asarray(base, dtype=np.float64)
    delta, allowed_d, x, allowed_x = _finish(tp, allowed_tp, base64, mask, box, bf16_operand)
    return dict(delta=delta, allowed_delta=allowed_d, x=x, allowed_x=allowed_x, t=t, scale=scale, mask=mask, eps=eps,
                raw=None if base64 is None else base64 + tp)


def random_start(B, per, sample0, seed, eps, ball, base=None, box=None, valid=None, bf16_operand=False):
    """One rmcl_pgd_random_start call: dict like step_ball's.  For the L-inf ball the float64 delta here, rounded to fp32, IS the
    kernel's value (one product of two fp32 numbers); `random_start_linf_f32` restates that case in fp32 arithmetic, box included."""
    mask = valid_mask(valid, B, per)
    eps = f32(eps)
    v = np.stack([start_draw(seed, sample0 + b, per) for b in range(B)])
    v = np.where(mask, v, 0.0)
    if ball == BALL_LINF:
        tp = eps * v
        allowed_tp = U * np.abs(tp)
    elif ball == BALL_L2:
        nrm = np.maximum(np.sqrt((v * v).sum(axis=1, keepdims=True)), f32(1e-12))
        tp = eps * v / nrm                              # product, quotient, fp32(norm): 3 u, one spare
        allowed_tp = 4 * U * np.abs(tp)
    else:
        raise ValueError(ball)
    base64 = None if base is None else np.asarray(base, dtype=np.float64)
    delta, allowed_d, x, allowed_x = _finish(tp, allowed_tp, base64, mask, box, bf16_operand)
    return dict(delta=delta, allowed_delta=allowed_d, x=x, allowed_x=allowed_x, mask=mask, eps=eps)


def random_start_linf_f32(B, per, sample0, seed, eps, base=None, box=None, valid=None):
    """The L-inf start in fp32 arithmetic, bit for bit what the kernel computes: (delta f32, x f32 or None)."""
    mask = valid_mask(valid, B, per)
    v = np.stack([start_draw(seed, sample0 + b, per) for b in range(B)]).astype(np.float32)      # exact
    delta = np.where(mask, np.float32(eps) * v, np.float32(0))
    if base is None:
        return delta, None
    base = np.asarray(base, dtype=np.float32)
    x = base + delta
    if box is not None:
        xc = np.minimum(np.maximum(x, np.float32(box[0])), np.float32(box[1]))
        x = np.where(mask, xc, x)
        delta = np.where(mask, x - base, np.float32(0))
    return delta.astype(np.float32), x.astype(np.float32)


def keep_worst(score_new, best_score, best_restart, restart, G, delta, best_delta, operand=None, best_operand=None):
    """One rmcl_pgd_keep_worst call on numpy arrays; returns the new (best_score, best_restart, best_delta, best_operand) and `take`."""
    score_new = np.asarray(score_new, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        take = np.ones(score_new.shape, dtype=bool) if restart == 0 else score_new > best_score
    rows = np.repeat(take, G)
    bs = np.where(take, score_new, best_score).astype(np.float32)
    br = np.where(take, np.int32(restart), best_restart).astype(np.int32)
    bd = np.where(rows[:, None], delta, best_delta)
    bo = None if operand is None else np.where(rows[:, None], operand, best_operand)
    return bs, br, bd, bo, take
