"""Reference, float32 emulation, comparison and case list for the optimizer kernels (csrc/optim.hip).  No GPU code: imported by
tests/test_optim_ref_host.py (CPU) and tests/test_gpu_optim_edges.py (GPU).

REFERENCE.  oracle.optim.adam_step / lamb_step in float64, one keras variable at a time, with the hyper-parameters passed AS THEIR
FLOAT32 VALUES (keras and the kernels both hold them in float32: with the plain doubles `1 - beta2` differs by 1.3e-5 relative,
which a tolerance would have to hide).

TWO-STAGE COMPARISON of ONE step, from the float32 state the step started from (no error accumulates over steps).  U = 2^-24.
  (a) m_new, v_new against the reference at the old float32 m, v, g:
        |m_new - m_ref| <= 4U (|b1 m| + |(1-b1) g|)      (relative to the sum of the ABSOLUTE terms: m cancels)
        |v_new - v_ref| <= 4U (b2 v + (1-b2) g^2)
      Roundings: b1*m, (1-b1)*g, the sum = 2.5U at most for m ((1 - b) is exact in float32 for b in [0.5, 1]); b2*v, (1-b2)*g, *g, the
      sum = 3.5U at most for v; fewer where the compiler fuses a product into the sum.
  (b) w_new against the float64 formula evaluated AT THE FLOAT32 m_new, v_new UNDER TEST (otherwise the cancellation error of m
      is divided by sqrt(v) + eps and no elementwise bound holds):
        |w_new - w_ref| <= 2U |w_ref| + K U |w_ref - w_old|,   K = 16 (Adam), 32 (LAMB)
      Adam: lr_t to float (0.5U), sqrtf (0.5U), + eps (0.5U), lr_t * m (0.5U), the quotient (0.5U): 2.5U on the step, and the final
      subtraction rounds w (0.5U |w|).  LAMB: 1/bc1, 1/bc2 to float, m * inv_bc1, v * inv_bc2 (halved by the root), sqrtf, + eps, the
      quotient, wd * w, the sum: <= 4U on the update; the update's norm inherits at most that, plus 16 squares summed per thread in
      float32 on the float4 path before the sums go to double (<= 16U on a sum, 8U on the ratio); two norms to float, their quotient,
      ratio * lr, * update: 2.5U.  Under 19U in all; half of K = 32 is the norm.
  `formula_matches_oracle` (host test) ties the stage-(b) formula to oracle.optim: at the oracle's own float64 m, v it gives the
  oracle's weights.

FLOAT32 EMULATION (`emulate`).  numpy float32, operation by operation in the kernels' order, with a `mutation=` argument.  It is
what the host test holds to the bounds above and what it breaks, one mutation at a time, to show that the case list catches each
of them through `compare`.  It is never the reference of a GPU test.
"""
import zlib

import numpy as np

from oracle import optim as o_opt

U = 2.0 ** -24
OPT_BLK = 4096                   # csrc/optim.hip: elements per work block
OPT_MAX_T = 48                   # csrc/optim.hip: tensors per launch
BOUND_M, BOUND_V = 4.0, 4.0      # in U of the absolute terms
K_W = {'adam': 16.0, 'lamb': 32.0}
KINDS = ('adam', 'lamb')


def f32(x):
    return float(np.float32(x))


class HP:
    """Hyper-parameters of one step: `raw` as the user writes them (doubles), the attributes as float32 VALUES held in doubles."""

    def __init__(self, kind, lr=None, b1=0.9, b2=0.999, eps=None, wd=1e-6):
        self.kind = kind
        if lr is None:
            lr = 1e-3 if kind == 'adam' else 0.25     # LAMB: a step comparable to the weights, so that w's final rounding cannot mask it
        if eps is None:
            eps = 1e-7 if kind == 'adam' else 1e-6
        self.raw = dict(lr=lr, b1=b1, b2=b2, eps=eps, wd=wd)
        self.lr, self.b1, self.b2, self.eps, self.wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)


class T:
    """One tensor of a step's table: float32 w, g, m, v (1-D), the length of one keras variable, and which of 'p', 'g', 'm', 'v'
    (at most one) the GPU test places 4 bytes into its allocation."""

    def __init__(self, w, g, m, v, var_len, misalign=None):
        self.w, self.g, self.m, self.v = (np.ascontiguousarray(a, np.float32).reshape(-1) for a in (w, g, m, v))
        self.var_len, self.misalign = int(var_len), misalign
        assert self.w.size % self.var_len == 0


class Case:
    def __init__(self, name, tensors, step=3, hp=None):
        self.name, self.tensors, self.step, self.hp_over = name, tensors, int(step), dict(hp or {})

    def hp(self, kind):
        return HP(kind, **self.hp_over)

    def __repr__(self):
        return self.name


# ---------------------------------------------------------------- reference ----------------------------------------------------------------
def ref_moments(kind, w, g, m, v, var_len, hp, step):
    """Stage (a): m, v of oracle.optim, one keras variable at a time, float64."""
    step_fn = o_opt.adam_step if kind == 'adam' else o_opt.lamb_step
    kw = dict(b1=hp.b1, b2=hp.b2, eps=hp.eps)
    if kind == 'lamb':
        kw['wd'] = hp.wd
    rows = [a.astype(np.float64).reshape(-1, var_len) for a in (w, g, m, v)]
    out = [step_fn(rows[0][k], rows[1][k], rows[2][k], rows[3][k], hp.lr, step, **kw) for k in range(rows[0].shape[0])]
    return (np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]), np.concatenate([o[2] for o in out]))


def ref_weights(kind, w_old, m_new, v_new, var_len, hp, step):
    """Stage (b): the weights of oracle.optim's formulas in float64, from GIVEN new moments."""
    w, m, v = (np.asarray(a, np.float64).reshape(-1, var_len) for a in (w_old, m_new, v_new))
    bc1, bc2 = 1 - hp.b1 ** step, 1 - hp.b2 ** step
    if kind == 'adam':
        return (w - hp.lr * np.sqrt(bc2) / bc1 * m / (np.sqrt(v) + hp.eps)).reshape(-1)
    u = (m / bc1) / (np.sqrt(v / bc2) + hp.eps) + hp.wd * w
    wn, un = np.linalg.norm(w, axis=1), np.linalg.norm(u, axis=1)
    ok = (wn > 0) & (un > 0)
    ratio = np.where(ok, wn / np.where(ok, un, 1.0), 1.0)
    return (w - ratio[:, None] * hp.lr * u).reshape(-1)


def _ratio(err, bound):
    """max err / bound; where the bound is 0 the value must be exact."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def compare(kind, old, new, var_len, hp, step):
    """old = (w, g, m, v), new = (w, m, v), float32 arrays of one tensor.  Returns the observed maxima in the units of the bounds:
    {'m': .. (bound BOUND_M), 'v': .. (BOUND_V), 'w': .. (K_W[kind])}; a value above its bound is a miss (inf: a value that had to be
    exact is not)."""
    w, g, m, v = (np.asarray(a, np.float32).reshape(-1) for a in old)
    wn, mn, vn = (np.asarray(a, np.float32).reshape(-1) for a in new)
    _, m_ref, v_ref = ref_moments(kind, w, g, m, v, var_len, hp, step)
    g64, m64, v64 = g.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    rm = _ratio(np.abs(mn - m_ref), U * (np.abs(hp.b1 * m64) + np.abs((1 - hp.b1) * g64)))
    rv = _ratio(np.abs(vn - v_ref), U * (hp.b2 * v64 + (1 - hp.b2) * g64 * g64))
    w_ref = ref_weights(kind, w, mn, vn, var_len, hp, step)
    # |w_new - w_ref| <= 2U |w_ref| + K U |step|, stated as: the excess over w's own rounding term, in U of the step, is at most K
    excess = np.maximum(np.abs(wn - w_ref) - 2 * U * np.abs(w_ref), 0.0)
    rw = _ratio(excess, U * np.abs(w_ref - w.astype(np.float64)))
    return {'m': rm, 'v': rv, 'w': rw}


def bounds(kind):
    return {'m': BOUND_M, 'v': BOUND_V, 'w': K_W[kind]}


def misses(kind, obs):
    b = bounds(kind)
    return [k for k in ('m', 'v', 'w') if not obs[k] <= b[k]]


# ---------------------------------------------------------------- float32 emulation ----------------------------------------------------------------
MUTATIONS = {                                    # name -> the optimizers it applies to
    'eps_inside_root': KINDS,                    # Adam: eps added to the BIAS-CORRECTED root (the torch placement); LAMB: eps under the root
    'eps_x10': KINDS,
    'eps_div10': KINDS,
    'no_weight_decay': ('lamb',),
    'weight_decay_after_norms': ('lamb',),
    'ratio_per_tensor': ('lamb',),               # one trust ratio per tensor instead of per variable
    'segment_off_by_one_variable': ('lamb',),    # the variable of element i looked up with numel / (n_vars + 1) for var_len
    'zero_norm_gives_0': ('lamb',),
    'no_bias_correction_v': ('lamb',),
    'adam_lr_t_without_sqrt_bc2': ('adam',),
    'last_partial_block_skipped': KINDS,         # the ragged last block of a multi-block tensor is not updated
    'double_hyper_parameters': KINDS,            # 1 - b from the plain doubles (1.3e-5 in v)
}


def _sumsq_float4_path(x):
    """sum x^2 over whole OPT_BLK blocks as lamb_moments_kernel's float4 path forms it: thread t of a block takes elements
    e*1024 + 4t .. + 3 for e = 0..3, 16 fused multiply-adds in float32, then everything in double."""
    q = x.reshape(-1, 4, 256, 4).transpose(0, 2, 1, 3).reshape(-1, 16).astype(np.float64)
    acc = np.zeros(q.shape[0], np.float32)
    for j in range(16):
        acc = (q[:, j] * q[:, j] + acc.astype(np.float64)).astype(np.float32)
    return float(acc.astype(np.float64).sum())


def _sumsq(x, float4_blocks):
    x = np.asarray(x, np.float32)
    n_full = (x.size // OPT_BLK) * OPT_BLK if float4_blocks else 0
    s = _sumsq_float4_path(x[:n_full]) if n_full else 0.0
    return s + float((x[n_full:].astype(np.float64) ** 2).sum())


def emulate(kind, w, g, m, v, var_len, hp, step, mutation=None, aligned=True):
    """One step in float32, in the order of the kernels of csrc/optim.hip.  Returns (w_new, m_new, v_new)."""
    assert mutation is None or kind in MUTATIONS[mutation], (kind, mutation)
    F = np.float32
    w, g, m, v = (np.asarray(a, F).reshape(-1) for a in (w, g, m, v))
    n = w.size
    b1, b2, lr, wd = F(hp.b1), F(hp.b2), F(hp.lr), F(hp.wd)
    eps = F(hp.eps * {'eps_x10': 10.0, 'eps_div10': 0.1}.get(mutation, 1.0))
    omb1, omb2 = F(1) - b1, F(1) - b2
    if mutation == 'double_hyper_parameters':
        omb1, omb2 = F(1.0 - hp.raw['b1']), F(1.0 - hp.raw['b2'])
    bc1, bc2 = 1.0 - float(b1) ** step, 1.0 - float(b2) ** step
    m_new = b1 * m + omb1 * g
    v_new = b2 * v + (omb2 * g) * g
    if kind == 'adam':
        if mutation == 'eps_inside_root':
            w_new = w - (F(float(lr) / bc1) * m_new) / (np.sqrt(v_new) / F(np.sqrt(bc2)) + eps)
        else:
            lr_t = F(float(lr) / bc1) if mutation == 'adam_lr_t_without_sqrt_bc2' else F(float(lr) * np.sqrt(bc2) / bc1)
            w_new = w - (lr_t * m_new) / (np.sqrt(v_new) + eps)
    else:
        inv1, inv2 = F(1.0 / bc1), F(1.0 if mutation == 'no_bias_correction_v' else 1.0 / bc2)
        root = np.sqrt(v_new * inv2 + eps) if mutation == 'eps_inside_root' else np.sqrt(v_new * inv2)
        u0 = (m_new * inv1) / (root + eps)
        u = u0 if mutation == 'no_weight_decay' else u0 + wd * w
        u_norm_of = u0 if mutation == 'weight_decay_after_norms' else u
        vl = n if mutation == 'ratio_per_tensor' else var_len
        n_vars = n // vl
        float4 = aligned and vl == n                    # vec_ok of lamb_moments_kernel: one variable, whole blocks, 16-byte aligned
        ratios = np.empty(n_vars, F)
        for s in range(n_vars):
            seg = slice(s * vl, (s + 1) * vl)
            wn, un = F(np.sqrt(_sumsq(w[seg], float4))), F(np.sqrt(_sumsq(u_norm_of[seg], float4)))
            ratios[s] = wn / un if (wn > 0 and un > 0) else F(0 if mutation == 'zero_norm_gives_0' else 1)
        idx = np.arange(n) // vl
        if mutation == 'segment_off_by_one_variable' and n_vars > 1:
            idx = np.minimum(np.arange(n) // max(1, n // (n_vars + 1)), n_vars - 1)
        w_new = w - (ratios[idx] * lr) * u
    if mutation == 'last_partial_block_skipped' and n > OPT_BLK and n % OPT_BLK:
        keep = slice((n // OPT_BLK) * OPT_BLK, n)
        w_new[keep], m_new[keep], v_new[keep] = w[keep], m[keep], v[keep]
    return w_new.astype(F), m_new.astype(F), v_new.astype(F)


# ---------------------------------------------------------------- cases ----------------------------------------------------------------
SINGLE_NUMELS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 4095, 4096, 4097, 8191, 8193, 3 * 4096 + 2050]
STACKED = [(128, 1), (128, 32), (128, 256), (64, 512), (256, 128),      # the last two: the stackings for EMB_SZ 64 and 256
           (6, 96),          # var_len % 32 == 0, not % 64, numel % 64 == 0: the half-wave path
           (3, 96),          # numel % 64 != 0: per-element atomics
           (7, 1000),        # variable boundaries in the middle of a wave
           (5, 4160),        # var_len > OPT_BLK: boundaries inside blocks
           (2, 4096), (130, 33)]
_FILL = [2, 6, 7, 9, 10, 11, 12, 13]
# (variables, var_len) per tensor.  Launch 1 = tensors 0..47: five stackings, 5x4160 and 2x4096, the single tensors up to 8191 (ragged
# multi-block: 4097, 8191, 5x4160) and fillers; launch 2 = tensors 48..59: 8193 and 3*4096+2050 (ragged multi-block), four stackings, fillers.
FULL_TABLE = ([STACKED[i] for i in (0, 1, 2, 3, 4, 8, 9)] + [(1, n) for n in SINGLE_NUMELS[:16]] + [(1, _FILL[i % 8]) for i in range(25)] +
              [(1, 8193), (1, 3 * 4096 + 2050)] + [STACKED[i] for i in (5, 6, 7, 10)] + [(1, _FILL[i % 8]) for i in range(6)])
COMPACT_TABLE = [(1, 1), (1, 5), (128, 1), (1, 65), (128, 32), (1, 257), (6, 96), (3, 96), (1, 4097), (7, 1000), (130, 33), (1, 8193),
                 (2, 4096), (5, 4160)]
assert len(FULL_TABLE) == 60 and FULL_TABLE[48] == (1, 8193)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _earlier_step(rng, n, scale):
    """m, v as one earlier step from zero leaves them, float32."""
    gp = (rng.normal(size=n) * scale).astype(np.float32)
    return np.float32(0.1) * gp, np.float32(0.001) * gp * gp


def make_tensor(rng, n_vars, var_len, regime, i=0, misalign=None):
    n = n_vars * var_len
    scale = 10.0 if i % 3 == 0 else 1.0
    w = rng.normal(size=n).astype(np.float32)
    g = (rng.normal(size=n) * scale).astype(np.float32)
    m, v = _earlier_step(rng, n, scale)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    if regime == 'eps':                                   # |g| log-uniform in [1e-9, 1e-5], m = v = 0 (step 1)
        g = (sign * 10.0 ** rng.uniform(-9, -5, n)).astype(np.float32)
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    elif regime == 'decay':                               # |w| about 1e5: wd * w is a tenth of the update at wd = 1e-6
        w = (sign * 1e5 * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    elif regime == 'g0':                                  # LAMB: update = wd w, ratio = 1 / wd, w_new = w (1 - lr)
        g, m, v = (np.zeros(n, np.float32) for _ in range(3))
    elif regime == 'w0':                                  # ratio = 1
        w = np.zeros(n, np.float32)
    elif regime == 'w0g0':                                # the weights stay exactly 0
        w, g, m, v = (np.zeros(n, np.float32) for _ in range(4))
    elif regime == 'zero_variable' and n_vars > 1:        # variable 1: w = 0 (ratio 1) next to non-zero neighbours ...
        w[var_len:2 * var_len] = 0
        if n_vars > 3:                                    # ... variable 2: nothing at all, stays exactly 0
            for a in (w, g, m, v):
                a[2 * var_len:3 * var_len] = 0
    else:
        assert regime in ('normal', 'zero_variable'), regime
    return T(w, g, m, v, var_len, misalign)


def make_table(name, shapes, regime):
    rng = _rng(name)
    return [make_tensor(rng, nv, vl, regime, i) for i, (nv, vl) in enumerate(shapes)]


def _misaligned(which):
    rng = _rng('misaligned_' + which)
    return [make_tensor(rng, 1, 8193, 'normal', 0, misalign=which), make_tensor(rng, 1, 5, 'normal', 1),
            make_tensor(rng, 3, 96, 'normal', 2)]


_CASES = None


def cases():
    """The case list of both tests (built once; treat as read-only)."""
    global _CASES
    if _CASES is None:
        c = [Case('full_table_60', make_table('full', FULL_TABLE, 'normal')),
             Case('table_48', make_table('t48', FULL_TABLE[:48], 'normal')),
             Case('table_49', make_table('t49', FULL_TABLE[:49], 'normal'))]
        c += [Case('misaligned_' + which, _misaligned(which)) for which in 'pgmv']
        c += [Case('eps_dominated', make_table('eps', COMPACT_TABLE, 'eps'), step=1),
              Case('decay_dominated', make_table('decay', COMPACT_TABLE, 'decay')),
              Case('wd_0p1_eps_1e-3', make_table('wd', COMPACT_TABLE, 'normal'), hp=dict(wd=0.1, eps=1e-3)),
              Case('zero_gradient', make_table('g0', COMPACT_TABLE, 'g0'), step=1),
              Case('zero_weights', make_table('w0', COMPACT_TABLE, 'w0')),
              Case('zero_weights_and_gradient', make_table('w0g0', COMPACT_TABLE, 'w0g0'), step=1),
              Case('zero_variable_in_stack', make_table('zv', COMPACT_TABLE, 'zero_variable'))]
        c += [Case(f'step_{s}', make_table(f'step{s}', COMPACT_TABLE, 'normal'), step=s) for s in (1, 2, 1000, 10 ** 6)]
        _CASES = c
    return _CASES


def case_ids():
    return [c.name for c in cases()]


def n_elements(case):
    return sum(t.w.size for t in case.tensors)
