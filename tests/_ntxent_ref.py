"""Float64 reference, a-priori error bounds, mutants and case list for the NT-Xent kernels (csrc/ntxent.hip).  Plain numpy, no GPU
code: imported by tests/test_ntxent_ref_host.py (CPU), tests/test_gpu_ntxent_edges.py and tests/_ntxent_worker.py (GPU).

REFERENCE.  `ref(org_all, rep_all, n_local, rank_offset, tau)` mirrors the contract of nafp_ntxent_forward (include/nafp.h): the
local rows R = [org_all[off:off+n_local] ; rep_all[off:off+n_local]] against the columns Z = [org_all ; rep_all]; per row
CE = LSE_{c != self(r)} S[r,c] - S[r,pos(r)] with S = R Z^T / tau.  tau enters AS ITS FLOAT32 VALUE (the C ABI takes a float:
0.05 and float32(0.05) differ by 1.5e-8 relative, 3e-7 on a logit of 20, which a bound would otherwise have to hide).
tests/test_ntxent_ref_host.py holds it to oracle/ntxent.py (compute_loss, grad_embeddings, replica_loss_fn) to 1e-12.

BOUNDS, term by term; u = 2^-24 (unit roundoff of float32).  Every bound is a function of the float64 quantities only.
  logit      |ds[r,c]| <= (d + 2) u sum_k |R_rk Z_ck| / tau         a length-d float32 dot product (any order) and the scaling by 1 / tau
  sim_mtx    the logit's bound
  exp        e_exp(x) = C_EXP u (1 + |x|), x the argument of the exponential.  C_EXP = 4.  Its source: AMD's public CDNA ISA
             reference gives V_EXP_F32 and V_LOG_F32 as accurate to 1 ULP, i.e. 2u relative (the hardware guides shipped with this
             project state no accuracy); forming the argument in float32 (the difference, the product with a rounded log2 e, in the
             backward a rounded log2 of the scale) costs at most 2u |x|; the online log-sum-exp replaces one exponential by a product
             of rescaling exponentials whose arguments add up to at most |x|, which doubles the |x| term.  Chosen once, before any
             kernel output was looked at.
  lse        |dlse[r]| <= max_c |ds[r,c]|  +  sum_c p[r,c] e_exp(s[r,c] - m_r)  +  DEPTH u  +  4u (|m_r| + |lse_r|) + 2u
             the row's largest logit error; the exponentials, weighted by the probabilities; the float32 sum of positive terms along
             its longest chain, DEPTH = 16 (inside a tile) + 2 (n_tiles + 8) (one addition and one rescaling product per tile for a
             wave that walks every tile, then the merges over lane halves, waves and splits); the logarithm (1 ULP of log2, the
             product with ln 2: 3u |lse - m| <= 3u (|m| + |lse|), 2u absolute near a sum of 1) and the final m + log(sum).
  row loss   |dlse[r]| + |ds[r,pos]| + u |loss_r|;  loss_sum: the rows' bounds (the rows are summed in double) + u |loss_sum|
  dS         dS[r,c] = (p[r,c] - [c == pos]) / n_global, x' = s - lse + log(1 / (tau n_global)) as the second-generation kernels form it:
             |ddS[r,c]| <= (p (|ds| + |dlse| + e_exp(|s - lse| + |log(tau n_global)|)) + 3u (p + [c == pos]) + 2^-126) / n_global
             (3u: the float32 scale 1 / (tau n_global), the product with it, the subtraction of the indicator; 2^-126: a flushed denormal)
  gradient   an entry is sum dS[r,c] V / tau over the rows that touch a column (n_terms = 2 n_local + 40) plus, for a local row, over
             all its columns (n_terms = 2 n_global + 40; 40: up to 32 split partials, the combine, the scaling):
             sum (|ddS| |V| + n_terms u |dS| |V|) / tau.   The symmetric single-device pass sums (dS + dS^T) Z in one chain of 2 n_global
             terms, which the two parts together cover.

MUTANTS.  `ref(..., mutate=NAME)` makes one deliberate error in the float64 computation of ONE row (`mutate_row`, default: the
middle `a` row; `tail_included`: the row that a leaked copy of column 0 changes most among the rows for which column 0 is neither
self nor positive -- a leaking clamp re-reads column 0 for every row, so the most affected ordinary row is what a test would see).
The host test asserts that every mutant leaves the bounds of the unmutated reference for every input set of the GPU tests.
"""
import functools
import zlib

import numpy as np

U = 2.0 ** -24
C_EXP = 4.0
MUTANTS = ('self_included', 'pos_shifted', 'tail_included', 'lse_of_neighbour', 'wrong_offset')
KINDS = ('loss', 'sim', 'grad')


class Ref:
    """loss_rows (2 n_local, ordered [a ; b]), loss_sum, sim (n_local, 2 n_global - 1), d_org / d_rep (n_global, d): this rank's
    contribution to the gradient of loss_sum / n_global; b_* the per-element bounds."""
    pass


def _drop(x, gi):
    """(n_local, n_global) -> (n_local, n_global - 1): row i without column gi[i]."""
    nl, ng = x.shape
    keep = np.ones((nl, ng), bool)
    keep[np.arange(nl), gi] = False
    return x[keep].reshape(nl, ng - 1)


def ref(org_all, rep_all, n_local, rank_offset, tau, mutate=None, mutate_row=None):
    assert mutate is None or mutate in MUTANTS, mutate
    A, B = np.asarray(org_all, np.float64), np.asarray(rep_all, np.float64)
    ng, d = A.shape
    nl, off = int(n_local), int(rank_offset)
    assert B.shape == (ng, d) and 0 < nl and 0 <= off and off + nl <= ng
    tau = float(np.float32(tau))
    Z = np.concatenate([A, B])
    R = np.concatenate([A[off:off + nl], B[off:off + nl]])
    n_rows, n_cols = 2 * nl, 2 * ng
    rows = np.arange(n_rows)
    is_b = rows >= nl
    gi = off + np.where(is_b, rows - nl, rows)
    home = np.where(is_b, ng + gi, gi)                     # where row r lives among the columns (never mutated)
    with np.errstate(all='ignore'):
        S = R @ Z.T / tau
        aS = np.abs(R) @ np.abs(Z).T / tau
        # ---- the unmutated softmax first: the default row of `tail_included` is chosen from it ----
        mr = mutate_row
        if mr is None:
            mr = nl // 2
            if mutate == 'tail_included':
                s0 = S[:, 0]
                v0 = np.ones((n_rows, n_cols), bool)
                v0[rows, home] = False
                sm0 = np.where(v0, S, -np.inf)
                lse0 = sm0.max(1) + np.log(np.exp(sm0 - sm0.max(1)[:, None]).sum(1))
                share = np.exp(s0 - np.logaddexp(lse0, s0))
                ordinary = (home != 0) & (np.where(is_b, gi, ng + gi) != 0)
                mr = int(np.argmax(np.where(ordinary, share, -1.0))) if ordinary.any() else 0
        gim = gi.copy()
        if mutate == 'wrong_offset':
            gim[mr] = (gim[mr] + 1) % ng
        self_col = np.where(is_b, ng + gim, gim)
        pos_col = np.where(is_b, gim, ng + gim)
        if mutate == 'pos_shifted':
            pos_col[mr] = (pos_col[mr] + 1) % n_cols
        valid = np.ones((n_rows, n_cols), bool)
        valid[rows, self_col] = False
        if mutate == 'self_included':
            valid[mr, self_col[mr]] = True
        Sm = np.where(valid, S, -np.inf)
        m = Sm.max(1)
        if mutate == 'tail_included':
            m[mr] = max(m[mr], S[mr, 0])
        E = np.exp(Sm - m[:, None])
        ssum = E.sum(1)
        if mutate == 'tail_included':
            ssum[mr] += np.exp(S[mr, 0] - m[mr])
        lse = m + np.log(ssum)
        lse_used = lse.copy()
        if mutate == 'lse_of_neighbour':
            lse_used[mr] = lse[(mr + 1) % n_rows]
        s_pos = S[rows, pos_col]
        o = Ref()
        o.loss_rows = lse_used - s_pos
        o.loss_sum = o.loss_rows.sum()
        o.sim = np.concatenate([S[:nl, ng:], _drop(S[:nl, :ng], gim[:nl])], 1)
        P = np.where(valid, np.exp(S - lse_used[:, None]), 0.0)
        ind = np.zeros((n_rows, n_cols))
        ind[rows, pos_col] = 1.0
        dS = (P - ind) / ng
        if mutate == 'tail_included':
            dS[mr, 0] += np.exp(S[mr, 0] - lse_used[mr]) / ng
        dZ = dS.T @ R / tau
        np.add.at(dZ, home, dS @ Z / tau)
        o.d_org, o.d_rep = dZ[:ng], dZ[ng:]
        # ---- bounds ----
        ds = (d + 2) * U * aS
        prob = E / ssum[:, None]
        x = np.where(valid, S - m[:, None], 0.0)
        n_tiles = (n_cols + 31) // 32
        depth = 16 + 2 * (n_tiles + 8)
        dlse = (np.where(valid, ds, 0.0).max(1) + (prob * C_EXP * U * (1 + np.abs(x))).sum(1) + depth * U +
                4 * U * (np.abs(m) + np.abs(lse)) + 2 * U)
        o.b_loss_rows = dlse + ds[rows, pos_col] + U * np.abs(o.loss_rows)
        o.b_loss_sum = o.b_loss_rows.sum() + U * abs(o.loss_sum)
        o.b_sim = np.concatenate([ds[:nl, ng:], _drop(ds[:nl, :ng], gim[:nl])], 1)
        xb = np.where(valid, np.abs(S - lse[:, None]), 0.0) + abs(np.log(tau * ng))
        ddS = np.where(valid, P * (ds + dlse[:, None] + C_EXP * U * (1 + xb)) + 3 * U * (P + ind) + 2.0 ** -126, 0.0) / ng
        adS = np.abs(dS)
        bZ = (ddS.T @ np.abs(R) + (n_rows + 40) * U * (adS.T @ np.abs(R))) / tau
        np.add.at(bZ, home, (ddS @ np.abs(Z) + (n_cols + 40) * U * (adS @ np.abs(Z))) / tau)
        o.b_d_org, o.b_d_rep = bZ[:ng], bZ[ng:]
    o.mutate_row = mr
    return o


def ratio(err, bound):
    """max err / bound; where the bound is 0 the value must be exact.  A NaN anywhere gives NaN (which fails `< 1`)."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    if err.size == 0:
        return 0.0
    if np.isnan(err).any():
        return float('nan')
    pos = bound > 0
    r = np.where(pos, err / np.where(pos, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def compare(got, want):
    """got: dict with any of 'loss' (the scalar loss_sum), 'sim', 'd_org', 'd_rep' (arrays).  Returns the worst error / bound per output
    kind present: {'loss': .., 'sim': .., 'grad': ..}."""
    out = {}
    if 'loss' in got:
        out['loss'] = ratio(abs(np.float64(got['loss']) - want.loss_sum), want.b_loss_sum)
    if 'sim' in got:
        out['sim'] = ratio(np.abs(np.asarray(got['sim'], np.float64) - want.sim), want.b_sim)
    if 'd_org' in got:
        out['grad'] = max(ratio(np.abs(np.asarray(got['d_org'], np.float64) - want.d_org), want.b_d_org),
                          ratio(np.abs(np.asarray(got['d_rep'], np.float64) - want.d_rep), want.b_d_rep), key=_nan_first)
    return out


def _nan_first(v):
    return np.inf if v != v else v


def as_outputs(r):
    """A reference's own outputs in the form `compare` takes (how the host test feeds a mutant to the unmutated bounds)."""
    return {'loss': r.loss_sum, 'sim': r.sim, 'd_org': r.d_org, 'd_rep': r.d_rep}


# ---------------------------------------------------------------- inputs ----------------------------------------------------------------
# Hard pairs: every embedding shares a common component of weight w, so all logits of a row are of one size and the softmax spreads
# over the whole row (with independent unit vectors the positive takes all the mass at tau <= 0.05 and a wrong column changes
# nothing a float32 bound can see).  b = a + 1.5 noise, as `_inputs.unit_pairs(noise=1.5)`.  w follows the temperature: the spread of
# the logits is that of the cosines divided by tau.
_COMMON = {0.01: 3.0, 0.05: 1.0, 0.5: 0.0, 1.0: 0.0}


@functools.lru_cache(maxsize=None)
def pairs(n, d=128, tau=0.05, variant='unit'):
    """variant: 'unit'; 'x3' (embeddings scaled by 3: logits up to 180 at tau = 0.05); 'dup' (exact duplicates, n >= 22);
    'nan' (one NaN element).  Returns read-only float32 arrays."""
    rng = np.random.default_rng(zlib.crc32(f'ntxent {n} {d} {tau} {variant}'.encode()))
    w = 3.0 if variant == 'x3' else _COMMON[tau]
    g = rng.normal(size=(n, d))
    if variant != 'x3':             # (at 9-fold logits such a column would take ALL the mass of every row and hide its own copy)
        g[0] *= 0.3                 # column 0 sits near the common component: a hard negative of EVERY row, because column 0 is what
    a = w * rng.normal(size=d) + g  # the kernels' clamp re-reads beyond a ragged tile -- a leak of it then moves every row's softmax
    b = a + 1.5 * rng.normal(size=(n, d))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    if variant == 'x3':
        a, b = 3 * a, 3 * b
    if variant == 'dup':
        a[5] = a[9]                 # a tie between two columns of every row, and two identical rows
        b[7] = a[7]                 # a positive that equals its anchor: its logit ties with the excluded self logit
        a[20] = a[21]
        b[20] = a[21]               # a[i] = b[i] = a[j]: a three-way tie at the row maximum
    a, b = a.astype(np.float32), b.astype(np.float32)
    if variant == 'nan':
        a[min(11, n - 1), 37 % d] = np.nan
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


class Case:
    def __init__(self, group, n, n_local=None, off=0, d=128, tau=0.05, variant='unit', clone=False):
        self.group, self.n, self.d, self.tau, self.variant = group, n, d, tau, variant
        self.n_local, self.off, self.clone = (n if n_local is None else n_local), off, clone

    @property
    def name(self):
        s = f'n{self.n}_d{self.d}'
        if (self.n_local, self.off) != (self.n, 0) or self.clone:
            s += f'_l{self.n_local}_o{self.off}' + ('_cloned' if self.clone else '')
        if self.tau != 0.05:
            s += f'_tau{self.tau}'
        return s + ('' if self.variant == 'unit' else '_' + self.variant)

    def __repr__(self):
        return self.name

    def inputs(self):
        return pairs(self.n, self.d, self.tau, self.variant)

    def ref(self, mutate=None):
        if mutate is None:
            return _cached_ref(self.n, self.d, self.tau, self.variant, self.n_local, self.off)
        a, b = self.inputs()
        return ref(a, b, self.n_local, self.off, self.tau, mutate=mutate)


@functools.lru_cache(maxsize=None)
def _cached_ref(n, d, tau, variant, n_local, off):
    """The unmutated reference of a case, computed once per process and shared by the tests (treat as read-only)."""
    a, b = pairs(n, d, tau, variant)
    return ref(a, b, n_local, off, tau)


GEOMETRY_N = (1, 2, 3, 16, 17, 32, 33, 64, 65, 521, 530)
GEOMETRY = [Case('geometry', n) for n in GEOMETRY_N] + [Case('geometry', n, d=d) for d in (64, 256) for n in (3, 33, 65, 530)]
PER_ROW = [Case('per_row', n, 1, off) for n in (33, 530) for off in sorted({0, 15, 16, 31, 32, n - 1})]
SHARDS = [Case('shards', 530, 77, 0), Case('shards', 530, 77, 300), Case('shards', 530, 77, 453), Case('shards', 530, 1, 529),
          Case('shards', 530, 530, 0, clone=True)]
COVER = [Case('cover', 530, 77, 0), Case('cover', 530, 200, 77), Case('cover', 530, 1, 277), Case('cover', 530, 252, 278)]
TEMPERATURE = [Case('temperature', n, tau=tau) for n in (33, 530) for tau in (0.01, 0.05, 0.5, 1.0)]
MAGNITUDE = [Case('magnitude', 33, variant='x3'), Case('magnitude', 33, variant='dup')]
NAN_CASE = Case('nan', 33, variant='nan')
DETERMINISM = Case('determinism', 530, 77, 300)
# the reduced table of the environment-selected paths (tests/_ntxent_worker.py)
WORKER = [Case('worker', n, d=d) for d in (64, 128) for n in (3, 65, 530)] + [Case('worker', 530, 77, 300, d=d) for d in (64, 128)]


def all_compared_cases():
    """Every case whose outputs a GPU test compares with the reference, once each."""
    seen, out = set(), []
    for c in GEOMETRY + PER_ROW + SHARDS + COVER + TEMPERATURE + MAGNITUDE + [DETERMINISM] + WORKER:
        key = (c.n, c.d, c.tau, c.variant, c.n_local, c.off)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def mutant_applies(case, mutant):
    """The combinations in which a mutant is the identity by the mathematics of the loss, whatever the inputs:
    n_global = 1: a row has one admissible column, so lse_a0 = s(a0, b0) = s(b0, a0) = lse_b0 and a neighbour's lse is the row's own;
    the offset wraps onto itself."""
    if case.n == 1 and mutant in ('lse_of_neighbour', 'wrong_offset'):
        return False
    return True


def mutant_kinds(case, mutant):
    """The output kinds in which a mutant has to show.  The gradient always; sim_mtx holds plain logits, so only the column map
    reaches it; the loss where it is a PER-ROW loss (n_local = 1: CE_a(i) + CE_b(i) of one anchor) -- the bound of a sum over many
    rows is the sum of their bounds and cannot see one row, which is why the GPU tests read single rows through n_local = 1."""
    kinds = ('loss', 'grad') if case.n_local == 1 else ('grad',)
    return kinds + ('sim',) if mutant == 'wrong_offset' else kinds
