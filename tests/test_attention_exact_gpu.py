"""Attention conformance on a real MI355X (csrc/attention.hip, csrc/attention_hd.hip through ops.attn_fwd / attn_fwd_split /
attn_bwd): exact mask geometry read off the outputs as integers, every output row against ref64 inside model64's envelope,
memory discipline (NaN behind every input, sentinels round every output) and the launchers' refusals.  The inputs, the two
references and the proofs of the integer recoveries are in tests/_attn_exact.py / tests/test_attention_exact_cpu.py.

Every launch here goes through `launch`: inputs sit in buffers with 70 pad rows before and after each sample and 8 pad columns
behind the heads, outputs are framed the same way with a sentinel pattern (gradients in [B, N, 3, D] buffers, so a stray write
lands in a neighbour's slot or in the frame), and every call checks the frames and that every owned element was written."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from egom2p_amd import _lib as L  # noqa: E402
from egom2p_amd import ops  # noqa: E402

import _attn_exact as X  # noqa: E402

DEV = "cuda"
G = 70                                  # pad / sentinel rows before and after every sample
CPAD = 8                                # pad / sentinel columns behind the heads of a row
SENT = 0x5A5A                           # bf16 bit pattern of the output frames (1.5e16: no result has it)
FSENT = 1.5e30                          # fp32 sentinel round LSE / DELTA / behind the split workspace
GF = 64                                 # fp32 sentinels on either side
NAN_BITS = 0x7FC0


class Frame:
    """int16 buffer [B, G + N + G, slots, H * P + CPAD] filled with `bits`; slot(s) hands out (pointer, batch stride, row stride)
    of rows G .. G + N of slot s and marks them owned"""

    def __init__(self, B, N, slots, H, P, bits):
        self.B, self.N, self.H, self.P, self.slots = B, N, H, P, slots
        self.ld = H * P + CPAD
        self.buf = torch.full((B, N + 2 * G, slots, self.ld), bits, dtype=torch.int16, device=DEV)
        self.own = torch.zeros(self.buf.shape, dtype=torch.bool, device=DEV)

    def slot(self, s):
        self.own[:, G:G + self.N, s, :self.H * self.P] = True
        return self.buf.data_ptr() + 2 * (G * self.slots + s) * self.ld, (self.N + 2 * G) * self.slots * self.ld, self.slots * self.ld

    def _rows(self, s):
        return self.buf.view(torch.bfloat16)[:, G:G + self.N, s, :self.H * self.P]

    def put(self, s, x):
        """x: [B, H, N, d] values, d <= P (the columns d .. P of a head are zero padding)"""
        B, H, N, d = x.shape
        t = torch.zeros(B, N, H, self.P, dtype=torch.bfloat16)
        t[..., :d] = x.permute(0, 2, 1, 3).to(torch.bfloat16)
        self._rows(s).copy_(t.reshape(B, N, H * self.P).to(DEV))

    def get(self, s):
        """[B, H, N, P] fp64 on the host"""
        return self._rows(s).reshape(self.B, self.N, self.H, self.P).permute(0, 2, 1, 3).double().cpu()

    def fill_frame(self, bits):
        self.buf[~self.own] = bits

    def check(self, bits, what, written=True):
        assert bool((self.buf[~self.own] == bits).all()), f"{what}: a write outside the rows it owns"
        if written:
            assert not bool((self.buf[self.own] == bits).any()), f"{what}: an owned element was not written"


class FFrame:
    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GF,), FSENT, dtype=torch.float32, device=DEV)

    @property
    def t(self):
        return self.buf[GF:GF + self.n]

    def check(self, what, written=True):
        assert bool((self.buf[:GF] == FSENT).all()) and bool((self.buf[GF + self.n:] == FSENT).all()), f"{what}: a write outside"
        if written:
            assert not bool((self.t == FSENT).any()), f"{what}: an element was not written"


def _i32(x):
    return torch.as_tensor(x).to(torch.int32).contiguous().to(DEV)


class Launch:
    """buffers and argument lists of one case; fwd() / split() / bwd() run the kernels and check the frames"""

    def __init__(self, c, pad_bits=0, seg=True):
        self.c = c
        B, H, Nq, Nk, d = c.dims
        self.P = P = c.hd[0] if c.hd else 64
        self.pad_bits = pad_bits
        self.qf, self.dof = Frame(B, Nq, 1, H, P, pad_bits), Frame(B, Nq, 1, H, P, pad_bits)
        self.kvf = Frame(B, Nk, 2, H, P, pad_bits)                   # packed [B, Nk, 2, D] like the engine's kv rows
        self.qf.put(0, c.q), self.dof.put(0, c.do), self.kvf.put(0, c.k), self.kvf.put(1, c.v)
        self.of, self.olof = Frame(B, Nq, 1, H, P, SENT), Frame(B, Nq, 1, H, P, SENT)
        self.same = Nq == Nk
        if self.same:                                               # packed [B, N, 3, D] gradients: dQ | dK | dV
            self.gq = self.gkv = Frame(B, Nq, 3, H, P, SENT)
            self.slots = (0, 1, 2)
        else:                                                       # dQ between two sentinel slots, dK and dV either side of one
            self.gq, self.gkv = Frame(B, Nq, 3, H, P, SENT), Frame(B, Nk, 3, H, P, SENT)
            self.slots = (1, 0, 2)
        self.lse, self.delta = FFrame(B * H * Nq), FFrame(B * H * Nq)
        per_row = c.ks.dim() == 2
        self.ks, self.ke = _i32(c.ks), _i32(c.ke)
        self.r = (Nq, 1) if per_row else (1, 0)
        self.kw = {}
        if c.hd:
            self.kw = dict(hd_pad=P, hd=d if c.hd[1] else None)
        if c.seg is not None and seg:
            self.kw = dict(seg=_i32(c.seg), seg_bad=None if c.seg_bad is None else _i32(c.seg_bad))
        self.sign = 1.0 if c.hd else -1.0                           # the d64 entries store MINUS lse2 / MINUS delta

    def fwd_args(self):
        c = self.c
        B, H, Nq, Nk, _ = c.dims
        k, v = self.kvf.slot(0), self.kvf.slot(1)
        a = dict(q=self.qf.slot(0), k=k, v=v, o=self.of.slot(0), lse=self.lse.t, ks=self.ks, ke=self.ke, r_bs=self.r[0], r_rs=self.r[1],
                 B=B, H=H, Nq=Nq, Nk=Nk, scale=c.scale)
        return a

    @staticmethod
    def _flat(a, names):
        out = []
        for n in names:
            out += list(a[n]) if isinstance(a[n], tuple) else [a[n]]
        return out

    def call_fwd(self, a, **kw):
        ops.attn_fwd(*self._flat(a, ("q", "k", "v", "o", "lse", "ks", "ke", "r_bs", "r_rs", "B", "H", "Nq", "Nk", "scale")), **kw)

    def call_split(self, a, splits, ws):
        ops.attn_fwd_split(*self._flat(a, ("q", "k", "v", "o", "lse", "ks", "ke", "r_bs", "r_rs", "B", "H", "Nq", "Nk", "scale")), splits, ws)

    def fwd(self):
        kw = dict(self.kw)
        if self.c.o_lo:
            kw["o_lo"] = self.olof.slot(0)[0]
        self.call_fwd(self.fwd_args(), **kw)
        torch.cuda.synchronize()
        self.of.check(SENT, "O"), self.lse.check("LSE")
        self.olof.check(SENT, "O_lo")
        out = dict(o=self.of.get(0), lse2=self.sign * self.lse.t.double().cpu().view(*self.c.dims[:3]))
        out["olo"] = self.olof.get(0) if self.c.o_lo else torch.zeros_like(out["o"])
        return out

    def split(self, splits):
        B, H, Nq, _, _ = self.c.dims
        n = ops.attn_fwd_split_floats(B, H, Nq, splits)
        ws = torch.full((n + GF,), FSENT, dtype=torch.float32, device=DEV)
        of, lse = Frame(B, Nq, 1, H, 64, SENT), FFrame(B * H * Nq)
        a = self.fwd_args()
        a["o"], a["lse"] = of.slot(0), lse.t
        self.call_split(a, splits, ws[:n])
        torch.cuda.synchronize()
        of.check(SENT, "split O"), lse.check("split LSE")
        assert bool((ws[n:] == FSENT).all()), "a write behind the split workspace"
        return dict(o=of.get(0), lse2=-lse.t.double().cpu().view(B, H, Nq), olo=torch.zeros(B, H, Nq, 64, dtype=torch.float64))

    def bwd_args(self):
        a = self.fwd_args()
        a.update(do=self.dof.slot(0), delta=self.delta.t, dq=self.gq.slot(self.slots[0]), dk=self.gkv.slot(self.slots[1]),
                 dv=self.gkv.slot(self.slots[2]))
        return a

    def call_bwd(self, a, **kw):
        ops.attn_bwd(*self._flat(a, ("q", "k", "v", "o", "do", "lse", "delta", "dq", "dk", "dv", "ks", "ke", "r_bs", "r_rs", "B", "H", "Nq",
                                     "Nk", "scale")), **kw)

    def bwd(self):
        """after fwd(): the forward's O / O_lo / LSE are the backward's inputs; their frames become input padding"""
        kw = dict(self.kw)
        if self.c.o_lo:
            kw["o_lo"] = self.olof.slot(0)[0]
            self.olof.fill_frame(self.pad_bits)
        self.of.fill_frame(self.pad_bits)
        self.call_bwd(self.bwd_args(), **kw)
        torch.cuda.synchronize()
        self.gq.check(SENT, "dQ"), self.gkv.check(SENT, "dK / dV"), self.delta.check("DELTA"), self.lse.check("LSE")
        self.of.check(self.pad_bits, "O (backward input)", written=False)
        return dict(dq=self.gq.get(self.slots[0]), dk=self.gkv.get(self.slots[1]), dv=self.gkv.get(self.slots[2]),
                    delta=self.sign * self.delta.t.double().cpu().view(*self.c.dims[:3]))

    def raw(self):
        """every owned output element as stored, for bit-for-bit comparisons"""
        return [f.buf[f.own] for f in (self.of, self.olof, self.gq, self.gkv)] + [self.lse.t.clone(), self.delta.t.clone()]


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def check_rows(name, got, ref, mod, key):
    """RMS(kernel - ref64) of every output row <= 2 x RMS(model64 - ref64) + 2^-9 x RMS(ref64): the factor 2 for fp32 summation
    order and the hardware exp2 / log2, the additive term for rows where the model lands on the reference."""
    d = ref.shape[-1]
    err, env = X.row_rms(got[..., :d] - ref), X.envelope(mod, ref, 2.0)
    ratio = (err / env.clamp_min(1e-300)).max().item()
    print(f"{name} {key}: worst row error / envelope = {ratio:.3f}")
    bad = err > env
    assert not bool(bad.any()), (name, key, "rows", bad.nonzero()[:5].tolist(), "error / envelope", ratio)
    if got.shape[-1] > d:
        assert bool((got[..., d:] == 0).all()), (name, key, "pad columns must be exactly 0")


def check_lse(name, out, ref, mod):
    lse = out["lse2"] * X.LN2
    tol = 2 * (mod["lse"] - ref["lse"]).abs() + 1e-5 * (1 + ref["lse"].abs())
    assert bool(((lse - ref["lse"]).abs() <= tol).all()), (name, "lse", ((lse - ref["lse"]).abs() / tol).max().item())


def check_forward(c, out, ref, mod, olo=True):
    check_rows(c.name, out["o"], ref["o"], mod["o"], "O")
    check_lse(c.name, out, ref, mod)
    if c.exact:
        t = X.exact_counts(c)
        n = t["n"][:, None, :, None].double()
        want = t["fwd"][:, None].expand(-1, c.dims[1], -1, -1)
        assert torch.equal(torch.round(out["o"][..., :64] * n).long(), want.long()), (c.name, "attended keys")
        assert torch.equal(torch.round(torch.exp2(out["lse2"])).long(), t["n"][:, None].expand(-1, c.dims[1], -1)), (c.name, "n from LSE")
        if c.o_lo and olo:
            hi = (out["o"] + out["olo"])[..., :64]
            assert bool(((hi - want / n).abs() <= 2.0 ** -15 * (want / n)).all()), (c.name, "O + O_lo")


def check_backward(c, fo, out, ref):
    """the envelope of the backward comes from model64 on the backward's own operands: the O, O_lo and LSE the forward stored
    (checked on their own by check_forward)"""
    d = c.dims[4]
    mod = X.model64(c.q, c.k, c.v, c.do, c.ks, c.ke, c.scale, c.o_lo, fwd=fo)
    for key in ("dq", "dk", "dv"):
        check_rows(c.name, out[key], ref[key], mod[key], key)
    # DELTA is the model's rule - rowsum(dO o O) or rowsum(dO o (O + O_lo)) - on the O the forward stored, up to the fp32
    # summation of 64 .. 128 products: 1e-5 x (1 + sum |dO o O|)
    terms = c.do * (fo["o"] + fo["olo"])[..., :d]
    assert bool(((out["delta"] - terms.sum(-1)).abs() <= 1e-5 * (1 + terms.abs().sum(-1))).all()), (c.name, "delta")
    zero_rows = c.do.abs().sum(-1) == 0
    assert bool((out["dq"][zero_rows] == 0).all()), (c.name, "zero dO rows must give exactly zero dQ rows")
    if c.exact:
        t = X.exact_counts(c)
        H = c.dims[1]
        assert bool((out["dk"] == 0).all()), (c.name, "dK must be exactly zero with Q = 0")
        dv, want = out["dv"][..., :64], t["dv"][:, None].expand(-1, H, -1, -1)
        # p = 1 / n and the stored dV are one bf16 rounding each
        assert bool(((dv - want).abs() <= want * (2 * X.U_BF16 + 2.0 ** -15)).all()), (c.name, "dV")
        if t["n_uniform"]:
            n = int(t["n"].flatten()[0])
            assert torch.equal(torch.round(dv * n).long(), t["bwd"][:, None].expand(-1, H, -1, -1).long()), (c.name, "attending queries")


# ---- 1 + 2: geometry and row-wise envelopes, forward and backward, NaN against zeros behind every input ---------------------
@pytest.mark.parametrize("name", X.case_names())
def test_forward_backward(name):
    c = X.get(name)
    ref, mod = X.reference(name)
    raws = []
    for bits in (0, NAN_BITS):
        run = Launch(c, pad_bits=bits)
        fo = run.fwd()
        bo = run.bwd()
        raws.append(run.raw())
        if bits == 0:
            check_forward(c, fo, ref, mod)
            check_backward(c, fo, bo, ref)
    # nothing behind Nk / Nq (or beside the heads) is read: NaN there leaves every stored bit as zeros there do
    for a, b in zip(*raws):
        assert torch.equal(a, b), (name, "padding was read")


@pytest.mark.parametrize("name", X.case_names(lambda c: c.seg is not None))
def test_row_groups_equal_the_per_row_launch(name):
    """the same intervals without `seg`: the recovered integers (and the envelopes) are those of the group launch"""
    c = X.get(name)
    ref, mod = X.reference(name)
    run = Launch(c, seg=False)
    fo = run.fwd()
    check_forward(c, fo, ref, mod)
    check_backward(c, fo, run.bwd(), ref)


@pytest.mark.parametrize("name,splits", [(c.name, s) for c in X.cases() for s in c.splits])
def test_split_keys(name, splits):
    c = X.get(name)
    ref, mod = X.reference(name)
    for bits in (0, NAN_BITS):
        out = Launch(c, pad_bits=bits).split(splits)
        check_forward(c, out, ref, mod, olo=False)


@pytest.mark.parametrize("name", ["geo-257x192-ragged-wg+iso", "geo-127x321-sample", "seg-300-tail", "hd68p96r-257x193-ragged",
                                  "rand-257x321-align64", "dyn-halves-129x321-partial"])
def test_two_launches_are_bit_identical(name):
    c = X.get(name)
    raws = []
    for _ in range(2):
        run = Launch(c)
        run.fwd(), run.bwd()
        raws.append(run.raw() + ([run.split(3)["o"]] if c.splits else []))
    for a, b in zip(*raws):
        assert torch.equal(a, b)


# ---- 4: refusals and no-ops -----------------------------------------------------------------------------------------------------
def _refused(fn):
    with pytest.raises(L.EgoHipError):
        fn()
    torch.cuda.synchronize()


def _bump(t, i, by):
    t = list(t)
    t[i] += by
    return tuple(t)


def _base(hd=None, **kw):
    return X.exact_case("refusal", 2, 2, 64, 64, "ragged", d=68 if hd else 64, hd=hd, **kw)


@pytest.mark.parametrize("hd", [None, (96, True)])
def test_refused_strides_and_pointers(hd):
    """Every stride off the 8-element grid and every output pointer off the 16-byte grid is EGO_ERR_ARG.  All buffers are fully
    allocated (70 rows of slack behind the last sample), so a missing refusal computes something wrong inside memory it owns."""
    c = _base(hd, o_lo=True)
    run = Launch(c)
    run.fwd()
    run.bwd()
    for t in ("q", "k", "v", "o"):
        for i in (1, 2):
            a = run.fwd_args()
            a[t] = _bump(a[t], i, 4)
            if t in "kv" and i == 2:                                  # keep k_rs == v_rs: that refusal is tested on its own
                a["k"], a["v"] = _bump(run.kvf.slot(0), 2, 4), _bump(run.kvf.slot(1), 2, 4)
            _refused(lambda: run.call_fwd(a, **run.kw))
    for t in ("q", "k", "v", "do", "dq", "dk", "dv", "o"):
        for i in (1, 2):
            a = run.bwd_args()
            a[t] = _bump(a[t], i, 4)
            if t in "kv" and i == 2:
                a["k"], a["v"] = _bump(run.kvf.slot(0), 2, 4), _bump(run.kvf.slot(1), 2, 4)
            _refused(lambda: run.call_bwd(a, **run.kw))
    a = run.fwd_args()
    a["o"] = _bump(a["o"], 0, 8)                                      # 8 bytes into a valid buffer
    _refused(lambda: run.call_fwd(a, **run.kw))
    _refused(lambda: run.call_fwd(run.fwd_args(), o_lo=run.olof.slot(0)[0] + 8, **run.kw))
    for t in ("dq", "dk", "dv"):
        a = run.bwd_args()
        a[t] = _bump(a[t], 0, 8)
        _refused(lambda: run.call_bwd(a, **run.kw))
    if not hd:                # k_rs != v_rs, both on the 8-element grid (the d64 kernels share the lane offsets of K and V)
        a = run.fwd_args()
        a["k"] = _bump(a["k"], 2, 8)
        _refused(lambda: run.call_fwd(a, **run.kw))
        a = run.bwd_args()
        a["v"] = _bump(a["v"], 2, 8)
        _refused(lambda: run.call_bwd(a, **run.kw))
    # nothing was launched: the outputs of the two good calls above are still in place, frames intact
    run.of.check(0, "O", written=False), run.gq.check(SENT, "dQ"), run.gkv.check(SENT, "dK / dV")


def test_refused_split_arguments():
    c = _base()
    run = Launch(c)
    B, H, Nq, _, _ = c.dims
    n17 = ops.attn_fwd_split_floats(B, H, Nq, 17)
    ws = torch.zeros(n17 + 8, dtype=torch.float32, device=DEV)
    _refused(lambda: run.call_split(run.fwd_args(), 17, ws))
    n4 = ops.attn_fwd_split_floats(B, H, Nq, 4)
    _refused(lambda: run.call_split(run.fwd_args(), 4, ws[:n4 - 1]))                  # too small (the memory behind it is ours)
    _refused(lambda: run.call_split(run.fwd_args(), 4, ws[1:n4 + 1]))                 # 4 bytes off the 16-byte grid
    _refused(lambda: run.call_split(run.fwd_args(), 4, None))
    assert bool((run.of.buf == SENT).all())
    run.call_split(run.fwd_args(), 4, ws[:n4])                                          # and the good call goes through
    torch.cuda.synchronize()


def test_refused_row_groups_and_head_pitch():
    c = X.get("seg-300-tail")
    run = Launch(c)
    a = run.fwd_args()
    a["Nk"] -= 1                                                                        # seg with Nq != Nk
    _refused(lambda: run.call_fwd(a, **run.kw))
    b = run.bwd_args()
    b["Nk"] -= 1
    _refused(lambda: run.call_bwd(b, **run.kw))
    for args, call in ((run.fwd_args(), run.call_fwd), (run.bwd_args(), run.call_bwd)):
        args["r_rs"] = 0                                                                # seg needs per-row intervals
        _refused(lambda: call(args, **run.kw))
        args["r_rs"], args["r_bs"] = 1, args["Nq"] - 8
        _refused(lambda: call(args, **run.kw))
    h = Launch(_base((128, False)))
    for pitch in (80, 112):                                                            # inside the buffers of pitch 128
        for hd in (68, None):
            _refused(lambda: h.call_fwd(h.fwd_args(), hd_pad=pitch, hd=hd))
            _refused(lambda: h.call_bwd(h.bwd_args(), hd_pad=pitch, hd=hd))
    assert bool((h.of.buf == SENT).all()) and bool((h.gq.buf == SENT).all())


def test_refused_backward_beyond_32768_rows():
    """the dK / dV kernel keeps one interval summary per 64-row query tile in LDS, 512 of them: Nq > 32768 is refused"""
    Nq = 32768 + 64
    c = X.Case("long", torch.zeros(1, 1, Nq, 64), torch.zeros(1, 1, 64, 64), torch.zeros(1, 1, 64, 64), torch.zeros(1, 1, Nq, 64),
               torch.zeros(1, Nq, dtype=torch.int64), torch.full((1, Nq), 64, dtype=torch.int64), 0.125)
    run = Launch(c)
    run.fwd()
    _refused(lambda: run.call_bwd(run.bwd_args()))
    assert bool((run.gq.buf == SENT).all()) and bool((run.gkv.buf == SENT).all()) and bool((run.delta.buf == FSENT).all())


@pytest.mark.parametrize("zero", ["B", "Nq"])
@pytest.mark.parametrize("hd", [None, (96, True)])
def test_empty_launches_return_success_and_write_nothing(zero, hd):
    c = _base(hd, o_lo=True)
    run = Launch(c)
    a, b = run.fwd_args(), run.bwd_args()
    a[zero] = b[zero] = 0
    run.call_fwd(a, o_lo=run.olof.slot(0)[0], **run.kw)
    run.call_bwd(b, o_lo=run.olof.slot(0)[0], **run.kw)
    if not hd:
        ws = torch.full((ops.attn_fwd_split_floats(2, 2, 64, 3),), FSENT, dtype=torch.float32, device=DEV)
        run.call_split(a, 3, ws)
        assert bool((ws == FSENT).all())
    torch.cuda.synchronize()
    for f in (run.of, run.olof, run.gq, run.gkv):
        assert bool((f.buf == SENT).all())
    assert bool((run.lse.buf == FSENT).all()) and bool((run.delta.buf == FSENT).all())
