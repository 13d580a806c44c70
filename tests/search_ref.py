"""Plain numpy references for the beam-search kernels (csrc/ctc_prefix.hip, csrc/beam.hip) and
the inputs their kernel tests share; no GPU code.

* `prefix_score_ref`: CTC prefix scoring (Algorithm 2 of Watanabe et al., "Hybrid CTC/attention
  architecture for end-to-end speech recognition") for one hypothesis and all its candidates,
  vectorised over the candidates and serial in t.  dtype=float64 is the reference; dtype=float32
  is the reference implementation's own arithmetic (np.logaddexp on f32), the noise floor the
  kernels are measured against.
* `initial_state_ref`, `extend_state_ref`, `chain_ref`: the forward variables of the empty
  prefix, their streaming extension, and of a prefix (the recursion chained along its labels).
* `prebeam_ref`, `select_ref`: the pre-beam and the beam selection in np.float32, one rounding
  per operation in the order beam.hip's header states, under the kernels' total orders.  Their
  results are integers and bit-reproducible f32 sums, so the comparison is exact.
* `rel_err`, `bound`: the metric |got - ref64| / (|ref64| + 1) and max(1e-6, 4 x floor).
* `ctc_logits`, `candidates`, `PrefixCase`: the inputs of the prefix-kernel tests.
"""
import numpy as np

LOGZERO = -10000000000.0
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------ prefix scores
def frame_range(T, ol, wstart=0, wend=0):
    """Frames [start, end) of the recursion: max(ol, 1) .. T, or the attention window."""
    end = min(wend, T) or T
    start = min(wstart or max(ol, 1), max(end, 1))
    return start, end


def initial_state_ref(logp, blank, dtype):
    """r0[t] = (logzero, sum of the blank log-probs of frames 0..t), summed in frame order."""
    x = np.asarray(logp, dtype=dtype)
    r = np.full((x.shape[0], 2), LOGZERO, dtype=dtype)
    r[:, 1] = np.cumsum(x[:, blank], dtype=dtype)
    return r


def extend_state_ref(logp, blank, r_old, T, dtype):
    """The first len(r_old) frames kept, r^n logzero and r^b accumulating the blank emissions
    from frame max(len(r_old), 1) on; an empty r_old starts from (logzero, logzero)."""
    x = np.asarray(logp, dtype=dtype)
    r = np.full((T, 2), LOGZERO, dtype=dtype)
    n = len(r_old)
    r[:n] = np.asarray(r_old, dtype=dtype)
    for t in range(max(n, 1), T):
        r[t, 1] = r[t - 1, 1] + x[t, blank]
    return r


def prefix_score_ref(logp, r_prev, ol, last, cands, blank, eos, dtype, wstart=0, wend=0):
    """logp (T, V), r_prev (T, 2): the forward variables r^n, r^b of the prefix g of ol labels
    ending in `last`; cands (n,).  Returns log_psi (n,) and the candidates' forward variables
    r (n, T, 2) of the prefixes g + c.

    Over frames [start, end) (frame_range), with log_phi[t] = r_prev^b[t] for a repeated label
    (ol > 0 and c == last) and logaddexp(r_prev^n[t], r_prev^b[t]) otherwise:
        r^n[t] = logaddexp(r^n[t-1], log_phi[t-1]) + logp[t, c]
        r^b[t] = logaddexp(r^n[t-1], r^b[t-1]) + logp[t, blank]
        psi    = logaddexp(psi, log_phi[t-1] + logp[t, c])
    from r[start-1] = logzero and psi = logzero, except the empty prefix (ol == 0), whose
    r[0] = (logp[0, c], logzero) and, when start == 1, psi = logp[0, c].  Every row outside
    [start, end) is logzero apart from that r[0].  <eos> takes logaddexp(r_prev[T-1]), blank
    takes logzero."""
    x = np.asarray(logp, dtype=dtype)
    rp = np.asarray(r_prev, dtype=dtype)
    cands = np.asarray(cands, dtype=np.int64)
    T, n = x.shape[0], len(cands)
    lz = dtype(LOGZERO)
    start, end = frame_range(T, ol, wstart, wend)
    xs, xb = x[:, cands], x[:, blank]
    r = np.full((T, 2, n), lz, dtype=dtype)
    if ol == 0:
        r[0, 0] = xs[0]
    r_sum = np.logaddexp(rp[:, 0], rp[:, 1])
    same = (cands == last) & (ol > 0)
    log_phi = np.where(same[None, :], rp[:, 1:2], r_sum[:, None])
    psi = xs[0].copy() if ol == 0 and start == 1 else np.full(n, lz, dtype=dtype)
    rn, rb = psi.copy(), np.full(n, lz, dtype=dtype)
    for t in range(start, end):
        nrn = np.logaddexp(rn, log_phi[t - 1]) + xs[t]
        nrb = np.logaddexp(rn, rb) + xb[t]
        psi = np.logaddexp(psi, log_phi[t - 1] + xs[t])
        rn, rb = nrn, nrb
        r[t, 0], r[t, 1] = rn, rb
    psi[cands == eos] = r_sum[T - 1]
    psi[cands == blank] = lz
    assert psi.dtype == dtype and r.dtype == dtype
    return psi, np.ascontiguousarray(r.transpose(2, 0, 1))


def chain_ref(logp, blank, eos, labels, dtype):
    """Forward variables (T, 2) of the prefix `labels`: the recursion chained along it from the
    initial state."""
    r = initial_state_ref(logp, blank, dtype)
    last = eos  # <sos>
    for k, y in enumerate(labels):
        _, rr = prefix_score_ref(logp, r, k, last, [y], blank, eos, dtype)
        r, last = rr[0], y
    return r


def rel_err(got, ref64):
    """max |got - ref64| / (|ref64| + 1)."""
    got, ref64 = np.asarray(got, dtype=F64), np.asarray(ref64, dtype=F64)
    if got.size == 0:
        return 0.0
    return float((np.abs(got - ref64) / (np.abs(ref64) + 1.0)).max())


def bound(floor):
    """The rule of test_lstm_train_kernels_gpu.py: 4 x the deviation from float64 of the same
    restatement in f32 on the case's own inputs, and no less than 1e-6."""
    return max(1e-6, 4.0 * floor)


# ------------------------------------------------------------------------------ beam selection
def weighted_ref(logp, w_dec, w_lb, use_lb):
    """W = w_dec * logp (+ w_lb) in f32, one rounding per operation."""
    W = F32(w_dec) * np.asarray(logp, dtype=F32)
    if use_lb:
        W = W + F32(w_lb)
    assert W.dtype == F32
    return W


def prebeam_ref(logp, w_dec, w_lb, use_lb, P, eos):
    """logp (n, V) f32 -> (n, P + 1) int32: per row the P best tokens of W (value descending,
    then token ascending), then <eos>."""
    W = weighted_ref(logp, w_dec, w_lb, use_lb)
    out = np.empty((W.shape[0], P + 1), dtype=np.int32)
    for h in range(W.shape[0]):
        out[h, :P] = np.argsort(-W[h], kind="stable")[:P]
        out[h, P] = eos
    return out


def select_ref(logp, cand, psi, prefix, score, w_dec, w_lb, use_lb, w_ctc, V, beam, T):
    """The new beam over the n * (P + 1) candidate slots.  logp (n, >= V) f32, cand and psi
    (n, P + 1), prefix and score (n,).
        W   = w_dec * logp[h, token] (+ w_lb)
        inc = psi - prefix[h]
        W   = (W + w_ctc * inc) + score[h]
    An <eos> slot (column P) whose token is among the hypothesis's P tokens is excluded.  Order:
    W descending, then the flat index h * V + token ascending.  Returns rec_i (beam, 4) =
    (parent, token, column, none), rec_f (beam, 4) = (W, decoder log-prob, inc, psi), last_next,
    rptr_next (the byte offset slot * T * 2 * 4 from the r_new base), prefix_next, score_next.
    With fewer valid slots than `beam` the remaining records have none = 1 and W = -inf (slot 0
    stands in for their other fields, which are unspecified)."""
    cand = np.asarray(cand, dtype=np.int64)
    n, P1 = cand.shape
    logp, psi = np.asarray(logp, dtype=F32), np.asarray(psi, dtype=F32).reshape(n, P1)
    prefix, score = np.asarray(prefix, dtype=F32), np.asarray(score, dtype=F32)
    lp = np.take_along_axis(logp, cand, 1)
    inc = psi - prefix[:, None]
    W = (weighted_ref(lp, w_dec, w_lb, use_lb) + F32(w_ctc) * inc) + score[:, None]
    assert W.dtype == F32 and inc.dtype == F32
    valid = np.ones((n, P1), dtype=bool)
    valid[:, P1 - 1] = [cand[h, P1 - 1] not in cand[h, :P1 - 1] for h in range(n)]
    valid &= W != -np.inf  # no score at all: never chosen
    flat = np.arange(n)[:, None] * V + cand
    slots = np.flatnonzero(valid.reshape(-1))
    order = slots[np.lexsort((flat.reshape(-1)[slots], -W.reshape(-1)[slots].astype(F64)))][:beam]
    rec_i = np.zeros((beam, 4), dtype=np.int32)
    rec_f = np.zeros((beam, 4), dtype=F32)
    rptr = np.zeros(beam, dtype=np.int64)
    for b in range(beam):
        none = b >= len(order)
        c = 0 if none else int(order[b])
        h, k = divmod(c, P1)
        rec_i[b] = (h, cand[h, k], k, int(none))
        rec_f[b] = (-np.inf if none else W[h, k], lp[h, k], inc[h, k], psi[h, k])
        rptr[b] = c * T * 2 * 4
    return dict(rec_i=rec_i, rec_f=rec_f, last_next=rec_i[:, 1].copy(), rptr_next=rptr,
                prefix_next=rec_f[:, 3].copy(), score_next=rec_f[:, 0].copy())


def quantised(shape, gen, scale=3.0, step=0.25):
    """f32 multiples of `step`: few distinct values, so exact ties are common."""
    return (np.round(gen.standard_normal(shape) * scale / step) * step).astype(F32)


# ------------------------------------------------------------------------------ kernel-test inputs
def ctc_logits(T, V, blank, seed, ld=None):
    """randn * 2 with the blank column raised by 2 (paths stay alive over hundreds of frames);
    padding columns up to ld are NaN: they are never read."""
    g = np.random.default_rng(seed)
    x = np.full((T, ld or V), np.nan, dtype=F32)
    x[:, :V] = g.standard_normal((T, V)) * 2
    x[:, blank] += 2
    return x


def candidates(V, n_hyp, n_cand, blank, eos, lasts, gen):
    """(n_hyp, n_cand) distinct tokens per hypothesis.  <eos>, blank and the hypothesis's own
    last label come first in an order rotated by the hypothesis, cut to n_cand, so every one of
    the three is among some hypothesis's candidates even at n_cand = 1; the rest is random and
    the whole list is shuffled."""
    out = np.empty((n_hyp, n_cand), dtype=np.int32)
    for h in range(n_hyp):
        forced = [eos, blank, int(lasts[h])]
        forced = (forced[h % 3:] + forced[:h % 3])[:n_cand]
        forced = list(dict.fromkeys(forced))
        rest = np.setdiff1d(np.arange(V), forced)
        row = np.concatenate([forced, gen.permutation(rest)[:n_cand - len(forced)]])
        out[h] = gen.permutation(row)
    return out


class PrefixCase:
    """One launch of the prefix kernels on the host: n_hyp parents, each the f64 recursion
    chained along a random prefix of ols[h] labels and rounded to f32, their candidates, and the
    f64 reference with the f32 floor, both reading the same f32 logp and parents as the kernel.
    logp (T, V) f32 is what ea_ctc_prefix_init wrote."""

    def __init__(self, logp, blank, eos, ols, n_cand, seed, wstart=0, wend=0):
        g = np.random.default_rng(seed)
        self.logp, self.blank, self.eos = logp, blank, eos
        self.T, self.V = logp.shape
        self.ols, self.n_hyp, self.n_cand = list(ols), len(ols), n_cand
        self.wstart, self.wend = wstart, wend
        labels = np.setdiff1d(np.arange(self.V), [blank, eos])
        self.prefixes = [g.choice(labels, size=ol).tolist() for ol in self.ols]
        self.lasts = np.array([p[-1] if p else eos for p in self.prefixes], dtype=np.int32)
        self.parents = [chain_ref(logp, blank, eos, p, F64).astype(F32) for p in self.prefixes]
        self.cands = candidates(self.V, self.n_hyp, n_cand, blank, eos, self.lasts, g)
        ref = [self._ref(h, F64) for h in range(self.n_hyp)]
        f32 = [self._ref(h, F32) for h in range(self.n_hyp)]
        self.psi64, self.r64 = np.stack([p for p, _ in ref]), np.stack([r for _, r in ref])
        self.psi32, self.r32 = np.stack([p for p, _ in f32]), np.stack([r for _, r in f32])
        self.floor = max(rel_err(self.psi32, self.psi64), rel_err(self.r32, self.r64))

    def _ref(self, h, dtype):
        return prefix_score_ref(self.logp, self.parents[h], self.ols[h], int(self.lasts[h]), self.cands[h],
                                self.blank, self.eos, dtype, self.wstart, self.wend)

    def dead_rows(self, h):
        """Mask (T,) of the frames outside [start, end)."""
        start, end = frame_range(self.T, self.ols[h], self.wstart, self.wend)
        t = np.arange(self.T)
        return (t < start) | (t >= end)
