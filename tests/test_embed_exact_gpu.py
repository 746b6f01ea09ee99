"""Conformance tests of the token front end of egom2p_amd/csrc/embed.hip on the GPU: ego_embed_fwd, ego_embed_bwd (embed_sums_kernel
and the atomic-free table scatter embed_tables_kernel), ego_reg_grad, ego_rows_compact / _gather / _scatter and ego_loss_perm.

Every buffer a kernel touches is an interior view of a larger allocation: input frames hold NaN bits, output frames a bit pattern no
result can be; after every call the frame must be untouched and every owned element of a pure output written.  Exact cases (small
integers, sums below 2^24) are compared bit for bit with int64 sums; numeric cases per element with an fp64 reference under the bound
gamma(n + 1) (|init| + sum |x_i|) of tests/_embed_ref.py.  tests/test_embed_exact_cpu.py proves on the host what this file relies on:
the geometry each case claims, the exactness, and that plain fp32 sums stay inside the bound."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _embed_ref as E  # noqa: E402
from egom2p_amd import _lib as L  # noqa: E402
from egom2p_amd import ops  # noqa: E402

DEV = "cuda"
F32, I32, U8 = torch.float32, torch.int32, torch.uint8
NAN, SENT, SENT_I, SENT_B = E.NAN_F32, E.SENT_F32, E.SENT_I32, E.SENT_U8


class Framed:
    """`view`: the owned middle of `buf`, lo elements (a multiple of four unless a case says otherwise) behind its start"""

    def __init__(self, shape, dtype, bits, lo, hi):
        n = int(np.prod(shape))
        self.buf = torch.empty(lo + n + hi, dtype=dtype, device=DEV)
        self.pattern = E.sbits(bits, self.buf.element_size())
        E.ibits(self.buf).fill_(self.pattern)
        self.view, self.lo, self.n = self.buf[lo:lo + n].view(shape), lo, n

    def frame_ok(self):
        b = E.ibits(self.buf)
        return bool((b[:self.lo] == self.pattern).all()) and bool((b[self.lo + self.n:] == self.pattern).all())

    def all_written(self):
        return not bool((E.ibits(self.view) == self.pattern).any())

    def host(self):
        return self.view.cpu()


def _margins(shape, lo, hi):
    w = 2 * shape[-1] if len(shape) > 1 else 16              # two rows round a matrix, 16 elements round a vector
    return (w if lo is None else lo), (w if hi is None else hi)


def put(host, bits=NAN, lo=None, hi=None):
    """the host tensor in a frame of `bits`"""
    host = torch.as_tensor(host)
    lo, hi = _margins(host.shape, lo, hi)
    f = Framed(tuple(host.shape), host.dtype, bits, lo, hi)
    f.view.copy_(host)
    return f


def blank(shape, dtype=F32, bits=SENT, lo=None, hi=None):
    """a pure output: sentinel everywhere"""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    lo, hi = _margins(shape, lo, hi)
    return Framed(shape, dtype, bits, lo, hi)


def same_bits(got, want, what):
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gb, wb = E.ibits(got), E.ibits(want)
    if not torch.equal(gb, wb):
        bad = (gb != wb).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ, first at {list(i)}: got {got[i].item()!r}, "
                             f"want {want[i].item()!r}")


# ================================================================================================================ ego_embed_bwd
class BwdState:
    def __init__(self, case, data, d2=True, dbase=True, touched=True):
        off = 1 if case["misalign"] else 0                   # one int32 off the 16-byte grid: the scalar key path
        self.case, self.rows, self.D = case, case["slot"].numel(), case["D"]
        self.slot, self.tok = put(case["slot"], lo=4 + off, hi=4), put(case["tok"], lo=4 + off, hi=4)
        assert self.slot.view.data_ptr() % 16 == 4 * off and self.tok.view.data_ptr() % 16 == 4 * off
        self.dx = put(data["dx"])
        self.d2 = put(data["d2"]) if d2 else None
        self.tab = [None if t is None else put(t, SENT) for t in data["tab"]]
        self.mod = [put(t, SENT) for t in data["mod"]]
        self.base = put(data["base"], SENT)
        self.use_base = dbase
        self.flags = [None if f is None else put(f, SENT_B) for f in data["touched"]] if touched else None
        self.inputs = [self.slot, self.tok, self.dx] + ([self.d2] if d2 else [])
        self.before = [f.buf.clone() for f in self.inputs]

    def outputs(self):
        return [t for t in self.tab if t is not None] + self.mod + [self.base] + [f for f in (self.flags or []) if f is not None]

    def call(self):
        v = lambda f: None if f is None else f.view           # noqa: E731
        ops.embed_bwd([v(t) for t in self.tab], [m.view for m in self.mod], self.base.view if self.use_base else None, self.dx.view,
                      v(self.d2), self.slot.view, self.tok.view, self.rows, self.D,
                      touched=None if self.flags is None else [v(f) for f in self.flags])

    def desc(self, work, work_floats):
        d = L.EmbedBwdDesc()
        for i, m in enumerate(self.mod):
            d.dtable[i] = None if self.tab[i] is None else self.tab[i].view.data_ptr()
            d.vocab[i] = 0 if self.tab[i] is None else self.tab[i].view.shape[0]
            d.dmod[i] = m.view.data_ptr()
            d.touched[i] = None if self.flags is None or self.flags[i] is None else self.flags[i].view.data_ptr()
        d.dbase = self.base.view.data_ptr()
        d.dx, d.d2 = self.dx.view.data_ptr(), self.d2.view.data_ptr()
        d.slot, d.tok = self.slot.view.data_ptr(), self.tok.view.data_ptr()
        d.rows, d.D, d.n_mods = self.rows, self.D, len(self.mod)
        d.work, d.work_floats = work.data_ptr(), work_floats
        return d

    def finish(self):
        """frames and inputs as they were; host copies of the results"""
        torch.cuda.synchronize()
        for f in self.outputs():
            assert f.frame_ok(), f"{self.case['name']}: written outside an output"
        for f, b in zip(self.inputs, self.before):
            assert torch.equal(E.ibits(f.buf), E.ibits(b)), f"{self.case['name']}: an input was changed"
        return dict(tab=[None if t is None else t.host() for t in self.tab], mod=[m.host() for m in self.mod], base=self.base.host(),
                    flags=None if self.flags is None else [None if f is None else f.host() for f in self.flags])


def run_bwd(case, data, calls, **opt):
    st = BwdState(case, data, **opt)
    for _ in range(calls):
        st.call()
    return st.finish()


def check_flags(case, data, got, got_row):
    """set exactly where a row received a contribution, beside the flags that were set before"""
    for m, want_row in enumerate(got_row):
        if want_row is not None:
            same_bits(got["flags"][m], torch.maximum(data["touched"][m], want_row.to(U8)), f"{case['name']} touched[{m}]")


def check_bwd_exact(case, opt=None, check_touched=True):
    opt = opt or {}
    data = E.bwd_data(case, True)
    want = E.bwd_expect_exact(case, data, 2, d2=opt.get("d2", True), dbase=opt.get("dbase", True))
    got = run_bwd(case, data, 2, **opt)                      # the entry point accumulates: twice
    for m in range(len(case["V"])):
        if want["tab"][m] is not None:
            same_bits(got["tab"][m], want["tab"][m], f"{case['name']} dtable[{m}]")
        else:
            assert got["tab"][m] is None
        same_bits(got["mod"][m], want["mod"][m], f"{case['name']} dmod[{m}]")
    same_bits(got["base"], want["base"], f"{case['name']} dbase")
    if check_touched:
        check_flags(case, data, got, want["got_row"])
    again = run_bwd(case, data, 2, **opt)                    # from scratch once more: bit for bit
    for a, b in zip(got["tab"] + got["mod"] + [got["base"]], again["tab"] + again["mod"] + [again["base"]]):
        if a is not None:
            same_bits(b, a, f"{case['name']} second run")
    return got


@pytest.mark.parametrize("name", E.BWD_EXACT)
def test_embed_bwd_exact(name):
    """integers: tables, modality sums and base equal int64 index_add_ / column sums bit for bit after two accumulating calls, the
    touched flags are the rows that received a contribution, a second run from scratch gives the same bits"""
    case = E.BWD_CASES[name][0]()
    check_bwd_exact(case)


@pytest.mark.parametrize("name", E.BWD_NUMERIC)
def test_embed_bwd_numeric(name):
    """randn: every element within gamma(n + 1) (|init| + sum |x_i|) of the fp64 reference, n the rows contributing to it"""
    case = E.BWD_CASES[name][0]()
    data = E.bwd_data(case, False)
    ref, bound = E.bwd_expect_numeric(case, data)
    got = run_bwd(case, data, 1)
    worst = 0.0
    items = [(f"dtable[{m}]", got["tab"][m], ref["tab"][m], bound["tab"][m]) for m in range(len(case["V"])) if ref["tab"][m] is not None]
    items += [(f"dmod[{m}]", got["mod"][m], ref["mod"][m], bound["mod"][m]) for m in range(len(case["V"]))]
    items += [("dbase", got["base"], ref["base"], bound["base"])]
    for what, g, r, b in items:
        err = (g.double() - r).abs()
        untouched = b == 0
        assert bool((err[untouched] == 0).all()), f"{name} {what}: an element no row contributes to has changed"
        ratio = float((err[~untouched] / b[~untouched]).max()) if bool((~untouched).any()) else 0.0
        worst = max(worst, ratio)
        print(f"{name} {what}: worst |got - ref| / bound = {ratio:.4f}")
        assert ratio <= 1.0, f"{name} {what}: |got - ref| is {ratio:.3f} x the bound"
    again = run_bwd(case, data, 1)
    for a, b in zip(got["tab"] + got["mod"] + [got["base"]], again["tab"] + again["mod"] + [again["base"]]):
        if a is not None:
            same_bits(b, a, f"{name} second run")


@pytest.mark.parametrize("opt", ["no_dbase", "no_d2", "no_touched", "touched"])
def test_embed_bwd_optional_arguments(opt):
    case = E.options_case()
    if opt == "touched":
        data = E.bwd_data(case, True)
        assert int(data["touched"][0].sum()) > 0             # flags already set stay set
        check_bwd_exact(case)
        return
    kw = dict(no_dbase=dict(dbase=False), no_d2=dict(d2=False), no_touched=dict(touched=False))[opt]
    check_bwd_exact(case, kw, check_touched=opt != "no_touched")   # dbase=None: the buffer keeps its values, checked bit for bit


def _work(n):
    return blank(n, F32, SENT, lo=16, hi=16)


@pytest.mark.parametrize("why", ["D%4", "D=2052", "n_mods=0", "n_mods=9", "work short", "65537 rows"])
def test_embed_bwd_refusals_leave_the_outputs_alone(why):
    """every refusal is raised through ops.check before anything is launched: tables, dmod, dbase and flags bit-unchanged"""
    case = E.options_case()
    if why == "65537 rows":
        case["V"][0] = 65537
    data = E.bwd_data(case, True)
    st = BwdState(case, data)
    snap = [f.buf.clone() for f in st.outputs()]
    lib = L.load()
    need = lib.ego_embed_bwd_work_floats(st.rows, st.D, len(st.mod))
    with pytest.raises(L.EgoHipError):
        if why == "65537 rows":
            st.call()
        else:
            work = _work(need)
            d = st.desc(work.view, need - 1 if why == "work short" else need)
            if why == "D%4":
                d.D = 126
            elif why == "D=2052":
                d.D = 2052
                work = _work(lib.ego_embed_bwd_work_floats(st.rows, 2052, len(st.mod)))
                d.work, d.work_floats = work.view.data_ptr(), work.n
            elif why.startswith("n_mods"):
                d.n_mods = int(why[-1])
            ops.check(lib.ego_embed_bwd(C.byref(d), torch.cuda.current_stream().cuda_stream), "ego_embed_bwd")
    torch.cuda.synchronize()
    for f, b in zip(st.outputs(), snap):
        assert torch.equal(E.ibits(f.buf), E.ibits(b)), f"{why}: a refused call changed an output"


def test_embed_bwd_work_exactly_as_asked():
    """the scratch the entry point asks for is enough: a buffer of exactly that size, framed, is not overrun (four-wave, one-wave and
    two-level column sums)"""
    lib = L.load()
    for case in (E.scan_case(2051), E.onewave_case(8, 1152, E.TWO_LEVEL_ROWS), E.flush_case()):
        data = E.bwd_data(case, True)
        st = BwdState(case, data)
        need = lib.ego_embed_bwd_work_floats(st.rows, st.D, len(st.mod))
        work = _work(need)
        ops.check(lib.ego_embed_bwd(C.byref(st.desc(work.view, need)), torch.cuda.current_stream().cuda_stream), "ego_embed_bwd")
        got = st.finish()
        assert work.frame_ok(), f"{case['name']}: the scratch was overrun"
        want = E.bwd_expect_exact(case, data, 1)
        for m in range(len(case["V"])):
            same_bits(got["tab"][m], want["tab"][m], f"{case['name']} dtable[{m}]")
            same_bits(got["mod"][m], want["mod"][m], f"{case['name']} dmod[{m}]")
        same_bits(got["base"], want["base"], f"{case['name']} dbase")


# ================================================================================================================ ego_embed_fwd
@pytest.mark.parametrize("variant", E.FWD_VARIANTS)
@pytest.mark.parametrize("D", E.FWD_DS)
def test_embed_fwd_bit_exact(D, variant):
    """x = tab + (pos + mod) and emb = pos + mod bit for bit; padding rows zeros, register rows x = reg[local] (zeros without reg),
    emb = 0; garbage local / tok of padding rows not looked up; tables in NaN frames; outputs over sentinels"""
    for rows in E.FWD_ROWS:
        c = E.fwd_case(D, rows, variant)
        want_x, want_e = E.fwd_ref(c)
        tabs = None if c["tables"] is None else [put(t) for t in c["tables"]]
        pos, mod = [put(t) for t in c["pos"]], [put(t) for t in c["mod"]]
        base = None if c["base_vec"] is None else put(c["base_vec"])
        reg = None if c["reg"] is None else put(c["reg"])
        slot, local, tok = (put(c[k], lo=4, hi=4) for k in ("slot", "local", "tok"))
        x = blank((rows, D))
        emb = None if variant == "noemb" else blank((rows, D))
        ops.embed_fwd(None if tabs is None else [t.view for t in tabs], [p.view for p in pos], [m.view for m in mod],
                      None if base is None else base.view, slot.view, local.view, tok.view, x.view, None if emb is None else emb.view,
                      rows, D, reg=None if reg is None else reg.view)
        torch.cuda.synchronize()
        what = f"D={D} rows={rows} {variant}"
        for name, f, want in (("x", x, want_x), ("emb", emb, want_e)):
            if f is None:
                continue
            assert f.frame_ok(), f"{what} {name}: written outside the rows"
            assert f.all_written(), f"{what} {name}: an owned element was not written"
            same_bits(f.host(), want, f"{what} {name}")
        pad = c["slot"] == -1
        assert not bool(x.host()[pad].any()), f"{what}: a padding row of x is not zero"


# ================================================================================================================ ego_reg_grad
@pytest.mark.parametrize("D", E.REG_DS)
@pytest.mark.parametrize("n_reg", E.REG_NS)
@pytest.mark.parametrize("B", E.REG_BS)
def test_reg_grad_bit_exact(B, n_reg, D):
    """dreg += sum over b ascending: integers twice (exact), randn once against the sequential fp32 sum on the host; the rows of dx that
    are not register rows hold NaN"""
    for exact, calls in ((True, 2), (False, 1)):
        c = E.reg_case(B, n_reg, D, exact)
        dx, dreg = put(c["dx"]), put(c["init"], SENT)
        for _ in range(calls):
            ops.reg_grad(dx.view, B, c["rps"], n_reg, D, dreg.view)
        torch.cuda.synchronize()
        assert dreg.frame_ok(), "written outside dreg"
        same_bits(dreg.host(), E.reg_ref(c, calls), f"B={B} n_reg={n_reg} D={D} {'exact' if exact else 'randn'}")


@pytest.mark.parametrize("why", ["n_reg > rows_per_sample", "D%4", "dx misaligned"])
def test_reg_grad_refusals_leave_dreg_alone(why):
    c = E.reg_case(3, 4, 1024, True)
    dx, dreg = put(c["dx"], hi=2 * 1024 + 4), put(c["init"], SENT)
    snap = dreg.buf.clone()
    with pytest.raises(L.EgoHipError):
        if why == "D%4":
            ops.reg_grad(dx.view, 3, c["rps"], 4, 1022, dreg.view)
        elif why == "dx misaligned":
            ops.reg_grad(dx.buf[dx.lo + 1:dx.lo + 1 + dx.n], 3, c["rps"], 4, 1024, dreg.view)
        else:
            ops.reg_grad(dx.view, 3, 3, 4, 1024, dreg.view)
    torch.cuda.synchronize()
    assert torch.equal(E.ibits(dreg.buf), E.ibits(snap)), f"{why}: a refused call changed dreg"


# ================================================================================================================ ego_rows_*
@pytest.mark.parametrize("pattern", E.ROWS_PATTERNS)
@pytest.mark.parametrize("V", E.ROWS_VS)
def test_rows_compact(V, pattern):
    """ascending list, -1 up to cap, the count word (bit 30 exactly when truncated), all flags cleared, nothing behind rows[cap]"""
    flags = E.compact_flags(V, pattern)
    count = int(np.count_nonzero(flags))
    for cap in E.compact_caps(count):
        want_rows, want_count = E.compact_ref(flags, cap)
        touched = put(torch.from_numpy(flags), SENT_B)
        rows, cnt = blank(cap, I32, SENT_I, lo=4, hi=4), blank(1, I32, SENT_I, lo=4, hi=4)
        ops.rows_compact(touched.view, cap, rows.view, cnt.view)
        torch.cuda.synchronize()
        what = f"V={V} {pattern} cap={cap}"
        assert rows.frame_ok() and cnt.frame_ok() and touched.frame_ok(), f"{what}: written outside a buffer"
        assert rows.all_written() and cnt.all_written(), f"{what}: an owned element was not written"
        same_bits(rows.host(), torch.from_numpy(want_rows), f"{what} rows")
        assert int(cnt.host()) == want_count, (what, hex(int(cnt.host())), hex(want_count))
        assert (want_count & E.TRUNC != 0) == (count > cap)
        assert not bool(touched.host().any()), f"{what}: a flag was not cleared"


def _count_words(cap):
    counts = sorted({0, 1, max(cap - 1, 0), cap})
    return [(n, n) for n in counts] + [(cap, cap | E.TRUNC)]           # a truncated list: bit 30 is masked off


@pytest.mark.parametrize("cap", E.ROWS_CAPS)
@pytest.mark.parametrize("D", E.ROWS_DS)
def test_rows_gather(D, cap):
    """out[i] = T[rows[i]] below count, zeros at and past it (the list holds rows of NaN there) and at -1 entries"""
    for n, word in _count_words(cap):
        table, rows, _ = E.rowlist_case(D, cap, n, "gather")
        T, r = put(torch.from_numpy(table)), put(torch.from_numpy(rows), lo=4, hi=4)
        cnt = put(torch.tensor([word], dtype=I32), lo=4, hi=4)
        out = blank((cap, D))
        ops.rows_gather(T.view, r.view, cnt.view, cap, out.view)
        torch.cuda.synchronize()
        what = f"D={D} cap={cap} count={word:#x}"
        assert out.frame_ok(), f"{what}: written outside out"
        assert out.all_written(), f"{what}: an owned element was not written"
        same_bits(out.host(), torch.from_numpy(E.gather_ref(table, rows, word, cap)), what)


@pytest.mark.parametrize("cap", E.ROWS_CAPS)
@pytest.mark.parametrize("D", E.ROWS_DS)
def test_rows_scatter(D, cap):
    """T[rows[i]] = (add ? T[rows[i]] : 0) + src[i] below count; src = None clears; -1 entries skipped; every other row of the table
    (NaN bits) and the frame bit-unchanged"""
    for (n, word), add, with_src in ((cw, a, s) for cw in _count_words(cap) for a in (0, 1) for s in (True, False)):
        table, rows, src = E.rowlist_case(D, cap, n, "scatter")
        T, r = put(torch.from_numpy(table), SENT), put(torch.from_numpy(rows), lo=4, hi=4)
        cnt = put(torch.tensor([word], dtype=I32), lo=4, hi=4)
        s = put(torch.from_numpy(src)) if with_src else None
        ops.rows_scatter(T.view, r.view, cnt.view, cap, None if s is None else s.view, add)
        torch.cuda.synchronize()
        what = f"D={D} cap={cap} count={word:#x} add={add} src={'given' if with_src else 'None'}"
        assert T.frame_ok(), f"{what}: written outside the table"
        same_bits(T.host(), torch.from_numpy(E.scatter_ref(table, rows, word, cap, src if with_src else None, add)), what)


# ================================================================================================================ ego_loss_perm
class LpState:
    def __init__(self, c):
        B, M, n = c["B"], c["M"], c["n_mods"]
        self.c = c
        self.ins = [put(torch.from_numpy(c[k].reshape(-1)), lo=4, hi=4) for k in ("seg", "canon", "slot", "tok")]
        self.perm, self.tgt = blank(B * M, I32, SENT_I), blank(B * M, I32, SENT_I)
        self.ranges, self.base = blank((n, 2), I32, SENT_I, lo=4, hi=4), blank((B, n), I32, SENT_I, lo=16, hi=16)

    def outs(self):
        return [self.perm, self.tgt, self.ranges, self.base]

    def call(self):
        c = self.c
        seg, canon, slot, tok = (f.view for f in self.ins)
        ops.loss_perm(seg, canon, slot, tok, c["B"], c["M"], c["n_mods"], self.perm.view, self.tgt.view, self.ranges.view, self.base.view)
        torch.cuda.synchronize()


def check_loss_perm(c, what):
    st = LpState(c)
    st.call()
    ref = E.lp_ref(c)
    for f in st.outs():
        assert f.frame_ok(), f"{what}: written outside an output"
    assert st.perm.all_written() and st.ranges.all_written() and st.base.all_written(), f"{what}: an owned element was not written"
    perm, tgt = st.perm.host().numpy(), st.tgt.host().numpy()
    kept = c["slot"] >= 0
    total = ref["total"]
    assert (perm[~kept] == -1).all(), f"{what}: a padding row has a place"
    assert np.array_equal(np.sort(perm[kept]), np.arange(total)), f"{what}: perm is not a bijection onto [0, total)"
    assert np.array_equal(tgt[perm[kept]], c["tok"][kept]), f"{what}: tgt_perm[perm[r]] != tok[r]"
    assert np.array_equal(perm, ref["perm"]), f"{what}: not the row order of y[decoder_mod_mask == id]"
    assert np.array_equal(tgt[:total], ref["tgt"])
    assert (tgt[total:] == st.tgt.pattern).all(), f"{what}: tgt_perm written past total"
    assert np.array_equal(st.ranges.host().numpy(), ref["ranges"]), f"{what}: ranges"
    assert np.array_equal(st.base.host().numpy(), ref["base"]), f"{what}: base"


def test_loss_perm_every_decoder_order():
    for order in E.LP_ORDERS:
        check_loss_perm(E.lp_case(2, 30, 4, order, "orders"), f"order {order}")


@pytest.mark.parametrize("n_mods", [1, 8])
def test_loss_perm_modality_counts(n_mods):
    canon = torch.randperm(n_mods, generator=E.gen("lp canon", n_mods)).tolist()
    check_loss_perm(E.lp_case(3, 40, n_mods, canon, "counts"), f"n_mods={n_mods}")


def test_loss_perm_empty_modality_and_padding_sample():
    check_loss_perm(E.lp_case(3, 30, 4, (2, 0, 3, 1), "empty", empty=2, pad_sample=1), "empty modality, padding sample")


@pytest.mark.parametrize("B,M", E.LP_SHAPES)
def test_loss_perm_shapes(B, M):
    """(37, 7100) is just above 256 workgroups x 1024 rows: the grid-stride loop runs"""
    check_loss_perm(E.lp_case(B, M, 4, (1, 3, 0, 2), "shapes"), f"B={B} M={M}")


def test_loss_perm_largest_lds_case_and_refusal():
    """3 B n_mods + 8 ints of LDS: B = 511 with eight modalities is the largest case under 48 KiB; B = 512 is refused, outputs untouched"""
    canon = (5, 0, 7, 2, 1, 6, 3, 4)
    check_loss_perm(E.lp_case(511, 16, 8, canon, "lds"), "B=511")
    st = LpState(E.lp_case(512, 16, 8, canon, "lds"))
    with pytest.raises(L.EgoHipError):
        st.call()
    torch.cuda.synchronize()
    for f in st.outs():
        assert bool((E.ibits(f.buf) == f.pattern).all()), "B=512: a refused call wrote an output"
