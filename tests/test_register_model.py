"""CPU: the host model of the register API (tests/register_model.py) and its sequence generator.

(a) the model composed of the project's restatements against plain linear algebra in numpy.longdouble: every gate an explicit
    2^n x 2^n matrix, every collapse a projector and a renormalisation, every marginal a plain sum.  This catches a model that is
    composed wrongly (qubit order, a collapse that forgets to scale, the inverse QFT on the wrong register); rounding is the
    business of the restatements' own tests.
(b) the generator reaches what it claims: every legal (state-setting kind, following kind) pair of each vocabulary at least
    three times over that vocabulary's seeds with nothing but quiet calls in between, judged on the op lists alone; the op lists
    of vocabulary 1 are the committed ones (tests/golden/sequence_digests.json); the Pauli calls of vocabulary 2 are not vacuous
    (masks of all three unit shapes, Y letters, values other than 0, non-finite states, rotations that change the state); the op
    lists of vocabulary 2 are pinned as well.  The same for vocabulary 3: its pairs, its op lists, batches whose terms share an
    x_mask and take a second read, density matrices of every width in all three kernel forms, and fused-engine knobs on
    registers large enough for them.
(c) the sharded family (register_model.generate_sharded): every legal pair of its own setting and following kinds at least three
    times, every refused entry point, every shard count and shape list; its op lists are the committed ones."""
import hashlib
import json
import os

import numpy as np
import pytest

import register_model as rm

LD, CLD = np.longdouble, np.clongdouble


# ---- (a) the long-double replay ----------------------------------------------------------------------------------------------

class Replay:
    def __init__(self, L, M):
        self.L, self.M, self.n = L, M, L + M
        self.dim = 1 << self.n
        self.v = np.zeros(self.dim, dtype=CLD)
        self.saved = {}

    def embed(self, U, qs, control=None):
        """the 2^n x 2^n matrix of U on the qubits qs (matrix index bit j = qubit qs[j]), identity where `control` reads 0"""
        G = np.zeros((self.dim, self.dim), dtype=CLD)
        for i in range(self.dim):
            if control is not None and not (i >> control) & 1:
                G[i, i] = 1
                continue
            row = sum(((i >> q) & 1) << j for j, q in enumerate(qs))
            base = i
            for q in qs:
                base &= ~(1 << q)
            for col in range(1 << len(qs)):
                G[i, base | sum(((col >> j) & 1) << q for j, q in enumerate(qs))] = U[row, col]
        return G

    def gate(self, U, qs, control=None):
        self.v = self.embed(np.asarray(U, dtype=CLD), qs, control) @ self.v

    def h(self, q):
        s = LD(1) / np.sqrt(LD(2))
        self.gate([[s, s], [s, -s]], [q])

    def cphase(self, c, t, theta):
        e = np.cos(LD(theta)) + 1j * np.sin(LD(theta))
        self.gate(np.diag(np.array([1, 1, 1, e], dtype=CLD)), [c, t])

    def camodc(self, Cn, atox, ctl):
        A, blk = atox % Cn, 1 << self.M
        G = np.zeros((self.dim, self.dim), dtype=CLD)
        for i in range(self.dim):
            f, dst = i & (blk - 1), i
            if (i >> ctl) & 1 and f < Cn:
                dst = (i & ~(blk - 1)) | (((A * f) % Cn) & (blk - 1))
            G[dst, i] += 1
        self.v = G @ self.v

    def iqft(self):
        for l in range(self.n - 1, self.M - 1, -1):
            self.h(l)
            for k in range(l - 1, self.M - 1, -1):
                self.cphase(l, k, np.pi / (1 << (l - k)))

    def qcomp(self, Cn, a):
        for l in range(self.M, self.n):
            self.h(l)
        x = a % Cn
        for l in range(self.M, self.n):
            self.camodc(Cn, x, l)
            x = (x * x) % Cn
        self.iqft()

    def probs(self):
        return self.v.real * self.v.real + self.v.imag * self.v.imag

    def marginal(self, first, num):
        p = self.probs().reshape(1 << (self.n - first - num), 1 << num, 1 << first)
        return p.sum(axis=(0, 2))

    def collapse(self, first, num, outcome):
        p = self.marginal(first, num)[outcome]
        keep = ((np.arange(self.dim) >> first) & ((1 << num) - 1)) == outcome
        self.v = np.where(keep, self.v, 0) / np.sqrt(p)
        return p

    def pauli(self, x_mask, z_mask):
        """the Pauli string as a 2^n x 2^n matrix: the Kronecker product of its letters, qubit 0 least significant; Y on x & z"""
        I, X = np.eye(2, dtype=CLD), np.array([[0, 1], [1, 0]], dtype=CLD)
        Y, Z = np.array([[0, -1j], [1j, 0]], dtype=CLD), np.array([[1, 0], [0, -1]], dtype=CLD)
        P = np.ones((1, 1), dtype=CLD)
        for q in range(self.n):
            xb, zb = (x_mask >> q) & 1, (z_mask >> q) & 1
            P = np.kron(Y if xb and zb else X if xb else Z if zb else I, P)
        return P

    def rdm(self, first, num):
        """rho[v, w] = sum over the other bits of amp[.., v, ..] conj(amp[.., w, ..]): interleaved (re, im) like rdm_ref"""
        x = self.v.reshape(1 << (self.n - first - num), 1 << num, 1 << first)
        rho = np.einsum("hvl,hwl->vw", x, np.conj(x))
        out = np.empty(rho.shape + (2,), dtype=LD)
        out[..., 0], out[..., 1] = rho.real, rho.imag
        return out

    def expect(self, x_mask, z_mask):
        return (np.conj(self.v) @ (self.pauli(x_mask, z_mask) @ self.v)).real

    def prot(self, x_mask, z_mask, theta):
        h = LD(theta) / LD(2)
        self.v = (np.cos(h) * np.eye(self.dim, dtype=CLD) - 1j * np.sin(h) * self.pauli(x_mask, z_mask)) @ self.v

    def interleaved(self):
        out = np.empty(2 * self.dim, dtype=LD)
        out[0::2], out[1::2] = self.v.real, self.v.imag
        return out


def index_is_consistent(p, r, idx, tol):
    """idx is what the reference's scan of the probabilities p gives for the draw r, up to `tol` on the running sums"""
    if r <= 0:
        return idx == 0
    cum = np.cumsum(p)[:-1]
    lo = int(np.searchsorted(cum, LD(r) - tol))
    hi = int(np.searchsorted(cum, LD(r) + tol))
    return min(lo, p.size - 1) <= idx <= min(hi, p.size - 1)


def replay_seed(ob, seed, bound):
    """the largest deviation of the model from the long-double replay over one small sequence"""
    cfg, ops = rm.generate(ob, seed, small=True, length=30)
    L, M, Cn, a = cfg.shapes[0]
    m, x = rm.RegisterModel(ob, L, M), Replay(L, M)
    worst = 0.0

    def near(got, want, what, scale=1.0):
        nonlocal worst
        d = float(np.max(np.abs(np.asarray(got, dtype=LD) - np.asarray(want, dtype=LD)))) / scale if np.size(got) else 0.0
        worst = max(worst, d)
        assert d <= bound, f"{cfg} op {i} {op!r}: {what} off by {d:.3e}\nops = {[o for _, o in ops[:i + 1]]!r}"

    for i, (_, op) in enumerate(ops):
        k = op[0]
        before = m.a.copy()
        got = rm.apply_to_model(m, op)
        if k in ("reset", "fill", "write", "load"):                       # data sources: the replay takes the model's doubles
            if k == "write":
                d = rm.window_data(m.dim, op[2], op[3], op[4])
                x.v[op[1]:op[1] + op[2]] = d[0::2].astype(LD) + 1j * d[1::2].astype(LD)
            elif k == "load":
                x.v = x.saved[op[1]].copy()
            else:
                x.v = m.a[0::2].astype(LD) + 1j * m.a[1::2].astype(LD)
                if k == "reset":
                    assert np.count_nonzero(m.a) == 1 and m.a[2] == 1.0
        elif k == "save": x.saved[op[1]] = x.v.copy()
        elif k == "h": x.h(op[1])
        elif k == "cphase": x.cphase(op[1], op[2], op[3])
        elif k == "camodc": x.camodc(op[1], op[2], op[3])
        elif k == "iqft": x.iqft()
        elif k == "qcomp": x.qcomp(op[1], op[2])
        elif k == "u1": x.gate(rm.matrix_data(2, op[2]), [op[1]])
        elif k == "cu1": x.gate(rm.matrix_data(2, op[3]), [op[2]], control=op[1])
        elif k == "u2": x.gate(rm.matrix_data(4, op[3]), [op[1], op[2]])
        elif k == "cu2": x.gate(rm.matrix_data(4, op[4]), [op[2], op[3]], control=op[1])
        elif k == "prot": x.prot(op[1], op[2], op[3])
        elif k == "expect": near(got, x.expect(op[1], op[2]), "expectation")
        elif k == "rdm":
            near(got[0], x.rdm(op[1], op[2]), "reduced density matrix")
            near(got[1], x.marginal(op[1], op[2]), "marginal")
        elif k in ("expect_sum", "expect_batch"):
            terms = (rm.sum_terms if k == "expect_sum" else rm.batch_terms)(m.n, op[1], op[2])
            values = [x.expect(xm, zm) for _, xm, zm in terms]
            near(got[1], values, "the values of the terms")
            # (the error of a sum grows at most linearly with its terms: the bound is that of the six terms an expect_sum op has at
            #  most, times k / 6 for the longer batches)
            near(got[0], sum((LD(c) * v for (c, _, _), v in zip(terms, values)), LD(0)), "the terms' sum", max(1.0, len(terms) / 6.0))
        elif k in ("read", "devptr"): near(got, x.interleaved()[2 * op[1]:2 * (op[1] + op[2])], "window")
        elif k == "marginal": near(got, x.marginal(op[1], op[2]), "marginal")
        elif k in ("total", "norm2"): near(got, x.probs().sum(), k)
        elif k == "measure":
            assert index_is_consistent(x.probs(), op[1], got, bound), (cfg, i, op, got)
            x.v[:] = 0
            x.v[got] = 1
        elif k == "sample":
            for r, idx in zip(rm.sample_draws(op[1], op[2]), got):
                assert index_is_consistent(x.probs(), r, int(idx), bound), (cfg, i, op, r, idx)
        elif k == "measure_qubits":
            v, p, st = got
            assert index_is_consistent(x.marginal(op[1], op[2]), op[3], v, bound), (cfg, i, op, got)
            near(p, x.marginal(op[1], op[2])[v], "probability")
            if st == rm.NO_ERROR:
                x.collapse(op[1], op[2], v)
            else:
                assert p == 0 and np.array_equal(m.a.view(np.uint64), before.view(np.uint64))
        elif k == "postselect":
            p, st = got
            near(p, x.marginal(op[1], op[2])[op[3]], "probability")
            if st == rm.NO_ERROR:
                x.collapse(op[1], op[2], op[3])
            else:
                assert p == 0 and np.array_equal(m.a.view(np.uint64), before.view(np.uint64))
        elif k == "refused":
            assert np.array_equal(m.a.view(np.uint64), before.view(np.uint64)), "a refused call changed the model"
        else:
            assert k in ("flush", "sync", "fusion", "stats", "stream"), op
        near(m.a, x.interleaved(), "state")
    return worst


SMALL_SEEDS = range(24)
# the largest deviation of the model from the long-double replay over SMALL_SEEDS is 1.110e-15 (amplitudes and probabilities of
# states of norm 1 to 4 after up to 30 calls, each of a few binary64 roundings); the bound is 16 times that: 1.776e-14
MEASURED, BOUND = 1.110e-15, 16 * 1.110e-15


# the same over SMALL_SEEDS_V2, the small sequences of vocabulary 2 (expectation values of up to 64 leaves, sums of up to six
# terms with coefficients below 2, rotations of one or two products per amplitude): 9.688e-16; the bound is 16 times that: 1.550e-14
SMALL_SEEDS_V2 = range(rm.SMALL_V1, 2 * rm.SMALL_V1)
MEASURED_V2, BOUND_V2 = 9.688e-16, 16 * 9.688e-16


# SMALL_SEEDS_V3, the small sequences of vocabulary 3, are held to vocabulary 2's bound: an entry of a density matrix is a sum of
# up to 64 products of two amplitudes, as a Pauli value is, and the sum of a batch of k terms is held to k / 6 times the bound of
# a sum of six (replay_seed)
SMALL_SEEDS_V3 = range(2 * rm.SMALL_V1, 3 * rm.SMALL_V1)
BOUND_V3 = BOUND_V2


def test_model_against_long_double_linear_algebra(ob):
    assert all(rm.Config(seed, small=True).vocab == 1 for seed in SMALL_SEEDS)
    worst = max(replay_seed(ob, seed, BOUND) for seed in SMALL_SEEDS)
    print(f"largest deviation of the model from the long-double replay: {worst:.3e} (bound {BOUND:.3e})")
    assert worst <= BOUND


def test_model_of_vocabulary_2_against_long_double_linear_algebra(ob):
    assert all(rm.Config(seed, small=True).vocab == 2 for seed in SMALL_SEEDS_V2)
    kinds = {op[0] for seed in SMALL_SEEDS_V2 for _, op in rm.generate(ob, seed, small=True, length=30)[1]}
    assert {"expect", "expect_sum", "prot", "devptr", "stream"} <= kinds
    worst = max(replay_seed(ob, seed, BOUND_V2) for seed in SMALL_SEEDS_V2)
    print(f"largest deviation of the model from the long-double replay, vocabulary 2: {worst:.3e} (bound {BOUND_V2:.3e})")
    assert worst <= BOUND_V2


def test_model_of_vocabulary_3_against_long_double_linear_algebra(ob):
    assert all(rm.Config(seed, small=True).vocab == 3 for seed in SMALL_SEEDS_V3)
    kinds = {op[0] for seed in SMALL_SEEDS_V3 for _, op in rm.generate(ob, seed, small=True, length=30)[1]}
    assert {"expect_batch", "rdm", "expect", "expect_sum", "prot", "devptr", "stream"} <= kinds
    worst = max(replay_seed(ob, seed, BOUND_V3) for seed in SMALL_SEEDS_V3)
    print(f"largest deviation of the model from the long-double replay, vocabulary 3: {worst:.3e} (bound {BOUND_V3:.3e})")
    assert worst <= BOUND_V3


def test_replay_notices_a_wrongly_composed_model(ob):
    """the replay is not vacuous: a model with the two-qubit gate's qubits swapped, or a postselect that does not scale, fails it;
    so do, on the sequences of vocabulary 2, an expectation with x_mask and z_mask swapped and a rotation by -theta, and on
    those of vocabulary 3 a density matrix that is transposed and a batch that answers its terms in reverse order"""
    class Swapped(rm.RegisterModel):
        def two_qubit_gate(self, q0, q1, U): super().two_qubit_gate(q1, q0, U)

    class Unscaled(rm.RegisterModel):
        def postselect(self, first, num, outcome):
            keep = ((np.arange(self.dim) >> first) & ((1 << num) - 1)) == outcome
            p = self.marginal(first, num)[outcome]
            self.a = np.where(np.repeat(keep, 2), self.a, 0.0)
            return p, rm.NO_ERROR

    class MasksSwapped(rm.RegisterModel):
        def expectation(self, x_mask, z_mask): return super().expectation(z_mask, x_mask)

    class Backwards(rm.RegisterModel):
        def pauli_rotation(self, x_mask, z_mask, theta): super().pauli_rotation(x_mask, z_mask, -theta)

    class Transposed(rm.RegisterModel):
        def reduced_density_matrix(self, first, num): return np.swapaxes(super().reduced_density_matrix(first, num), 0, 1)

    class Reversed(rm.RegisterModel):
        def expectation_batch(self, terms):
            total, values = super().expectation_batch(terms)
            return total, values[::-1]

    for broken, seeds, bound in ((Transposed, SMALL_SEEDS_V3, BOUND_V3), (Reversed, SMALL_SEEDS_V3, BOUND_V3), (Swapped, SMALL_SEEDS, BOUND), (Unscaled, SMALL_SEEDS, BOUND),
                                 (MasksSwapped, SMALL_SEEDS_V2, BOUND_V2), (Backwards, SMALL_SEEDS_V2, BOUND_V2)):
        real, rm.RegisterModel = rm.RegisterModel, broken
        try:
            with pytest.raises(AssertionError):
                for seed in seeds:
                    replay_seed(ob, seed, bound)
        finally:
            rm.RegisterModel = real


# ---- (b) what the generator reaches ----------------------------------------------------------------------------------------------

_GENERATED = {}


def generated(ob, seed):
    """(Config, ops) of one seed, generated once per session"""
    if seed not in _GENERATED:
        _GENERATED[seed] = rm.generate(ob, seed)
    return _GENERATED[seed]


def test_generator_reaches_every_pair(ob):
    for vocab in (1, 2, 3):
        pairs_of_vocabulary(ob, vocab)


def pairs_of_vocabulary(ob, vocab):
    total, lengths, calls = {}, [], {}
    seeds, following = rm.seeds_of(vocab), rm.following_of(vocab)
    for seed in seeds:
        cfg, ops = generated(ob, seed)
        assert cfg.vocab == vocab
        assert eval(repr(ops)) == ops, "an op list must replay from its printed form"
        mine = [op for which, op in ops if which == 0]
        lengths.append(len(mine))
        for pair, cnt in rm.pairs_reached(cfg.shapes[0], cfg.mode, mine, vocab).items():
            total[pair] = total.get(pair, 0) + cnt
        full = sum(1 for op in mine if op[0] == "read" and op[2] == 1 << (cfg.shapes[0][0] + cfg.shapes[0][1]))
        assert mine[-1][0] == "read" and full <= len(mine) // 3, (seed, full, len(mine))
        if cfg.compact:
            assert not any(op[0] == "devptr" for op in mine), "a handed-out pointer ends the compact chains run_ops asserts"
        for _, op in ops:
            calls[op[0]] = calls.get(op[0], 0) + 1
    legal = [(s, f) for s in rm.SETTING for f in following
             if any(rm.pair_is_legal(s, f, rm.Config(k).shapes[0], rm.Config(k).compact) for k in seeds)]
    print(f"vocabulary {vocab}, seeds {seeds[0]} .. {seeds[-1]}; ops per seed: {min(lengths)} .. {max(lengths)}")
    print(" " * 20 + " ".join(f"{f[:6]:>6}" for f in following))
    for s in rm.SETTING:
        print(f"{s:20}" + " ".join(f"{total.get((s, f), 0):6d}" if (s, f) in legal else "     -" for f in following))
    print("calls: " + ", ".join(f"{k} {calls.get(k, 0)}" for k in following))
    short = [(p, total.get(p, 0)) for p in legal if total.get(p, 0) < 3]
    assert not short, f"pairs reached fewer than 3 times: {short}"
    # all but (write of an Inf/NaN, norm2) and, from vocabulary 2 on, (compact, devptr)
    assert len(legal) == len(rm.SETTING) * len(following) - min(vocab, 2)
    assert (len(rm.SETTING), len(following)) == (11, {1: 25, 2: 30, 3: 32}[vocab])
    assert 40 <= min(lengths) and max(lengths) <= {1: 90, 2: 140, 3: 150}[vocab], lengths   # (a circuit front alone is L + a few calls)


def test_vocabulary_1_generates_the_committed_op_lists(ob):
    """the seeds below NSEEDS_V1 (and the small seeds below SMALL_V1) are frozen: sha256 of repr(ops), recorded with the generator
    as it was before vocabulary 2 existed.  What these seeds assert on the GPU cannot drift when the generator grows."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sequence_digests.json")) as f:
        golden = json.load(f)
    assert sorted(golden["big"], key=int) == [str(s) for s in range(rm.NSEEDS_V1)]
    assert sorted(golden["small"], key=int) == [str(s) for s in range(rm.SMALL_V1)]
    digest = lambda ops: hashlib.sha256(repr(ops).encode()).hexdigest()
    drifted = [s for s in range(rm.NSEEDS_V1) if digest(generated(ob, s)[1]) != golden["big"][str(s)]]
    drifted += [("small", s) for s in range(rm.SMALL_V1) if digest(rm.generate(ob, s, small=True, length=30)[1]) != golden["small"][str(s)]]
    assert not drifted, f"the op lists of these vocabulary-1 seeds changed: {drifted}"


def test_pauli_calls_of_vocabulary_2_are_not_vacuous(ob):
    """on the model alone, over the seeds of vocabulary 2: what the expect and prot ops meet"""
    ex = dict(n=0, x=0, y=0, nonzero=0, nonfinite=0, shape=[0, 0, 0])
    pr = dict(n=0, changed=0, shape=[0, 0, 0])
    for seed in rm.seeds_of(2):
        cfg, ops = generated(ob, seed)
        models = [rm.RegisterModel(ob, L, M) for L, M, _, _ in cfg.shapes]
        for which, op in ops:
            m = models[which]
            if op[0] == "expect":
                ex["nonfinite"] += m.holds_nonfinite()
            before = m.a
            got = rm.apply_to_model(m, op)
            if op[0] == "expect":
                ex["n"] += 1
                ex["x"] += op[1] != 0
                ex["y"] += (op[1] & op[2]) != 0
                ex["nonzero"] += got != 0                                  # (a NaN is a value other than 0)
                ex["shape"][rm.mask_shape(op[1])] += 1
            elif op[0] == "prot":
                pr["n"] += 1
                pr["changed"] += not np.array_equal(before.view(np.uint64), m.a.view(np.uint64))
                pr["shape"][rm.mask_shape(op[1])] += 1
    print(f"expect: {ex}\nprot: {pr}")
    assert 2 * ex["x"] >= ex["n"], "at least half of the expect ops have x_mask != 0"
    assert 5 * ex["y"] >= ex["n"], "at least a fifth carry a Y"
    assert 2 * ex["nonzero"] >= ex["n"], "at least half return a value other than 0"
    assert 10 * ex["nonfinite"] >= ex["n"], "at least a tenth fall on a non-finite state"
    assert 10 * pr["changed"] >= 9 * pr["n"], "at least 90 % of the prot ops change the bits of the state"
    assert min(ex["shape"]) >= 20 and min(pr["shape"]) >= 20, "each of the three unit shapes in >= 20 expect and >= 20 prot ops"


def test_new_calls_of_vocabulary_3_are_not_vacuous(ob):
    """on the model alone, over the seeds of vocabulary 3: what the expect_batch and rdm ops meet, which refused forms occur and
    which knobs the seeds run under"""
    eb = dict(n=0, shared=0, two_reads=0, nonzero=0, nonfinite=0, shape=[0, 0, 0], k={})
    rd = dict(n=0, offdiag=0, nonfinite=0, shape=[0, 0, 0], num=[0] * (rm.RDM_MAX + 1))
    refused, drawn, plain = {}, set(), []
    for seed in rm.seeds_of(3):
        cfg, ops = generated(ob, seed)
        assert cfg.vocab == 3
        fused = {k: v for k, v in cfg.knobs.items() if k.startswith(("fuse_", "meas_"))}
        if fused:
            assert seed % 3 and all(L + M >= max(M + 6, 10) for L, M, _, _ in cfg.shapes), cfg
            assert not (cfg.compact and set(fused) & set(rm.ENDS_COMPACT_CHAINS)), cfg
            drawn |= {i for i, d in enumerate(rm.KNOBS_FUSED) if all(fused.get(k) == v for k, v in d.items())}
        if not cfg.knobs:
            plain.append(seed)
        models = [rm.RegisterModel(ob, L, M) for L, M, _, _ in cfg.shapes]
        for which, op in ops:
            m = models[which]
            bad = m.holds_nonfinite()
            got = rm.apply_to_model(m, op)
            if op[0] == "expect_batch":
                terms = rm.batch_terms(m.n, op[1], op[2])
                xs = [x for _, x, _ in terms]
                eb["n"] += 1
                eb["k"][op[2]] = eb["k"].get(op[2], 0) + 1
                eb["shared"] += len(terms) >= 2 and len(set(xs)) == 1
                eb["two_reads"] += any(xs.count(x) > rm.BATCH_WIDTH for x in set(xs))
                eb["nonzero"] += got[0] != 0
                eb["nonfinite"] += bad
                for x in set(xs):
                    eb["shape"][rm.mask_shape(x)] += 1
                assert np.array_equal(got[1].view(np.uint64), m.expectation_sum(terms)[1].view(np.uint64))
            elif op[0] == "rdm":
                rho, P = got
                rd["n"] += 1
                rd["num"][op[2]] += 1
                rd["shape"][rm.rdm_shape(m.n, op[1], op[2])] += 1
                rd["offdiag"] += bool(np.any(rho[~np.eye(1 << op[2], dtype=bool)] != 0))
                rd["nonfinite"] += bad
                assert rho.shape == (1 << op[2], 1 << op[2], 2) and P.shape == (1 << op[2],)
            elif op[0] == "refused" and op[1][0] in ("rdm", "expect_batch"):
                refused[(op[1][0], op[2])] = refused.get((op[1][0], op[2]), 0) + 1
                if op[1][0] == "rdm":
                    past = op[1][1] + op[1][2] > m.n
                    assert op[2] == (rm.BAD_QUBIT if past else rm.UNSUPPORTED) and (past or op[1][2] > rm.RDM_MAX), op
    print(f"expect_batch: {eb}\nrdm: {rd}\nrefused: {refused}\nfused-engine knob dicts drawn: {sorted(drawn)}; seeds without knobs: {plain}")
    assert 3 * eb["shared"] >= eb["n"], "at least a third of the batches have two or more terms that all share one x_mask"
    assert eb["two_reads"] >= 10, "batches with more than BATCH_WIDTH terms on one x_mask: a second read of the state"
    assert set(eb["k"]) == {0, 1, 3, 6, 40} and eb["k"][0] >= 3 and min(v for k, v in eb["k"].items() if k) >= 10
    assert 2 * eb["nonzero"] >= eb["n"] and 20 * eb["nonfinite"] >= eb["n"]
    assert min(eb["shape"]) >= 20 and min(rd["shape"]) >= 20, "every mask shape and every form of the density-matrix kernel >= 20 times"
    assert min(rd["num"]) >= 20, "every width 0 .. RDM_MAX at least 20 times"
    assert 2 * rd["offdiag"] >= rd["n"] - rd["num"][0] and 20 * rd["nonfinite"] >= rd["n"]
    assert all(refused.get(key, 0) >= 3 for key in (("rdm", rm.BAD_QUBIT), ("rdm", rm.UNSUPPORTED), ("expect_batch", rm.BAD_QUBIT))), refused
    assert drawn == set(range(len(rm.KNOBS_FUSED))), "every dict of KNOBS_FUSED is drawn by some seed"
    # what tests/test_gpu_concurrent_callers.py picks from: seeds that run under the default knobs
    assert any(len(rm.Config(s).shapes) == 1 and not rm.Config(s).compact for s in plain) and len(plain) >= 16


def test_vocabulary_3_generates_the_committed_op_lists(ob):
    """the seeds NSEEDS .. NSEEDS_V3 - 1 and the small seeds 2 SMALL_V1 .. 3 SMALL_V1 - 1 are frozen like the others"""
    golden = golden_digests()
    assert sorted(golden["big_v3"], key=int) == [str(s) for s in rm.seeds_of(3)]
    assert sorted(golden["small_v3"], key=int) == [str(s) for s in SMALL_SEEDS_V3]
    drifted = [s for s in rm.seeds_of(3) if digest(generated(ob, s)[1]) != golden["big_v3"][str(s)]]
    drifted += [("small", s) for s in SMALL_SEEDS_V3 if digest(rm.generate(ob, s, small=True, length=30)[1]) != golden["small_v3"][str(s)]]
    assert not drifted, f"the op lists of these vocabulary-3 seeds changed: {drifted}"
    # the digest covers the op lists; the knobs a seed runs under are part of what the GPU asserts, so they are pinned too
    knobs = hashlib.sha256(repr([sorted(rm.Config(s).knobs.items()) for s in rm.seeds_of(3)]).encode()).hexdigest()
    assert knobs == golden["knobs_v3"], "the knobs of the vocabulary-3 seeds changed"


def test_generator_is_deterministic(ob):
    assert rm.generate(ob, 3)[1] == rm.generate(ob, 3)[1]
    assert rm.generate(ob, 3)[1] != rm.generate(ob, 4)[1]
    assert rm.generate(ob, 70)[1] == rm.generate(ob, 70)[1]


def golden_digests():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sequence_digests.json")) as f:
        return json.load(f)


def digest(ops):
    return hashlib.sha256(repr(ops).encode()).hexdigest()


def test_vocabulary_2_generates_the_committed_op_lists(ob):
    """the seeds NSEEDS_V1 .. NSEEDS - 1 and the small seeds SMALL_V1 .. 2 SMALL_V1 - 1 are frozen like those of vocabulary 1:
    what the GPU asserts for them cannot drift when the generator grows"""
    golden = golden_digests()
    assert sorted(golden["big_v2"], key=int) == [str(s) for s in rm.seeds_of(2)]
    assert sorted(golden["small_v2"], key=int) == [str(s) for s in SMALL_SEEDS_V2]
    drifted = [s for s in rm.seeds_of(2) if digest(generated(ob, s)[1]) != golden["big_v2"][str(s)]]
    drifted += [("small", s) for s in SMALL_SEEDS_V2 if digest(rm.generate(ob, s, small=True, length=30)[1]) != golden["small_v2"][str(s)]]
    assert not drifted, f"the op lists of these vocabulary-2 seeds changed: {drifted}"


# ---- (c) the sharded family ----------------------------------------------------------------------------------------------------------

_SHARDED = {}


def sharded(ob, seed):
    if seed not in _SHARDED:
        _SHARDED[seed] = rm.generate_sharded(ob, seed)
    return _SHARDED[seed]


def test_sharded_family_reaches_every_pair(ob):
    """the reach table of the 48 seeds (3274 ops, 48 .. 93 a seed): the fewest times a legal pair is reached is 3; 53 % of the
    Hadamard ops fall on one of the top k + 1 qubits and 77 % of the partial windows straddle a shard boundary; every refused
    entry point occurs 12 to 23 times; 20 ordinary, 20 tiny and 8 compact seeds, 18 / 15 / 15 seeds on 2 / 4 / 8 shards"""
    total, lengths, calls, refused, lists, counts = {}, [], {}, {}, {}, {}
    hs, windows = [0, 0], [0, 0]
    for seed in range(rm.NSEEDS_SH):
        cfg, ops = sharded(ob, seed)
        assert eval(repr(ops)) == ops, "an op list must replay from its printed form"
        mine = [op for _, op in ops]
        lengths.append(len(mine))
        lists[cfg.kind] = lists.get(cfg.kind, 0) + 1
        counts[cfg.shards] = counts.get(cfg.shards, 0) + 1
        assert cfg.shape in rm.SH_SHAPES[cfg.kind][cfg.shards]
        assert (cfg.n_local < 2 * cfg.k + 6) == (cfg.kind == "tiny"), cfg
        assert cfg.compact or cfg.kind != "compact", cfg
        for pair, cnt in rm.sh_pairs_reached(cfg, mine).items():
            total[pair] = total.get(pair, 0) + cnt
        full = sum(1 for op in mine if op[0] == "read" and op[2] == 1 << cfg.n)
        assert mine[-1] == ("read", 0, 1 << cfg.n) and full <= len(mine) // 3, (seed, full, len(mine))
        per = 1 << cfg.n_local
        for op in mine:
            calls[op[0]] = calls.get(op[0], 0) + 1
            if op[0] == "h":
                hs[0] += 1
                hs[1] += op[1] >= cfg.n - cfg.k - 1
            elif op[0] in ("read", "write") and op[2] < 1 << cfg.n:
                windows[0] += 1
                windows[1] += op[1] // per != (op[1] + op[2] - 1) // per
            elif op[0] == "refused":
                refused[op[1][0]] = refused.get(op[1][0], 0) + 1
                assert op[2] == (rm.BAD_QUBIT if op[1][0] in ("h", "cphase") else rm.UNSUPPORTED)
            elif op[0] == "fusion":
                assert op[1] in (-1, 0, 1), "no mode 2"
            elif op[0] == "write":
                assert op[4] in ("plain", "negzero"), "no Inf / NaN writes on a sharded register"
    cfgs = [rm.ShardedConfig(k) for k in range(rm.NSEEDS_SH)]
    legal = [(s, f) for s in rm.SETTING_SH for f in rm.FOLLOWING_SH if any(rm.sh_pair_is_legal(s, f, c) for c in cfgs)]
    print(f"sharded family, seeds 0 .. {rm.NSEEDS_SH - 1}; ops per seed: {min(lengths)} .. {max(lengths)}, {sum(lengths)} in all")
    print(" " * 20 + " ".join(f"{f[:6]:>6}" for f in rm.FOLLOWING_SH))
    for s in rm.SETTING_SH:
        print(f"{s:20}" + " ".join(f"{total.get((s, f), 0):6d}" if (s, f) in legal else "     -" for f in rm.FOLLOWING_SH))
    print("calls: " + ", ".join(f"{k} {calls.get(k, 0)}" for k in rm.FOLLOWING_SH))
    print(f"refused: {refused}\nH ops {hs[0]}, on the top k + 1 qubits {hs[1]}; partial windows {windows[0]}, across a shard boundary {windows[1]}")
    print(f"shape lists {lists}, shard counts {counts}; fewest times a legal pair is reached: {min(total.get(p, 0) for p in legal)}")
    short = [(p, total.get(p, 0)) for p in legal if total.get(p, 0) < 3]
    assert not short, f"pairs reached fewer than 3 times: {short}"
    assert len(legal) == len(rm.SETTING_SH) * len(rm.FOLLOWING_SH) and (len(rm.SETTING_SH), len(rm.FOLLOWING_SH)) == (10, 21)
    assert all(refused.get(j, 0) >= 2 for j in rm.REFUSED_SH + ("h", "cphase")), refused
    assert all(lists.get(k, 0) >= 6 for k in rm.SH_SHAPES) and all(counts.get(w, 0) >= 6 for w in (2, 4, 8))
    assert {(c.kind, c.shards) for c in cfgs} >= {(k, w) for k in rm.SH_SHAPES for w in (2, 4, 8)}
    assert 3 * hs[1] >= hs[0], "at least a third of the Hadamards target one of the top k + 1 qubits"
    assert 2 * windows[1] >= windows[0], "at least half of the partial windows straddle a multiple of 2^n_local"
    assert 40 <= min(lengths) and max(lengths) < 100, lengths
    assert any(c.kind == "compact" and c.relays and c.shards == 8 for c in cfgs), "a compact seed whose relay is really set up"
    assert {c.kind for c in cfgs if c.relays} == set(rm.SH_SHAPES) and sum(1 for c in cfgs if c.relays) == rm.NSEEDS_SH // 6
    assert sum(1 for c in cfgs if c.kind == "compact" and not c.relays) >= 3, "compact seeds that start without relays"
    assert max(c.n for c in cfgs) <= 16
    assert sum(1 for c in cfgs if "QCX_SHARD_FORCE_STAGED" in c.env) == rm.NSEEDS_SH // 6
    edges = {op[1] for seed in range(rm.NSEEDS_SH) for _, op in sharded(ob, seed)[1] if op[0] == "measure" and isinstance(op[1], str)}
    assert edges == set(rm.MEASURE_EDGES), edges


def test_sharded_family_generates_the_committed_op_lists(ob):
    golden = golden_digests()
    assert sorted(golden["sharded"], key=int) == [str(s) for s in range(rm.NSEEDS_SH)]
    drifted = [s for s in range(rm.NSEEDS_SH) if digest(sharded(ob, s)[1]) != golden["sharded"][str(s)]]
    assert not drifted, f"the op lists of these seeds of the sharded family changed: {drifted}"


def test_sharded_generator_is_deterministic(ob):
    assert rm.generate_sharded(ob, 7)[1] == rm.generate_sharded(ob, 7)[1]
    assert rm.generate_sharded(ob, 7)[1] != rm.generate_sharded(ob, 8)[1]
    assert repr(rm.ShardedConfig(7)) == repr(rm.ShardedConfig(7))
