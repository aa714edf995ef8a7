"""GPU: the fused BatchNorm-GEMM layer kernels of the training stacks, ONE layer at a time through the C ABI, against the float64
references of tests/_stack_layer_cases.py: pn2x_tg_fwd / pn2x_tg_fwd2 (csrc/train_gemm.hip, train_fwd.hip), pn2x_tg_bwd_slice in
both kernel variants with slices and pair launches (train_bwd.hip), pn2x_tg_dgrad / pn2x_tg_wgrad / pn2x_tg_reduce_multi.

The tolerance rule, everywhere: distance from float64 <= max(F, 4 x E_torch) (_train_cases.bound).  F is the floor of a length-L
fp32 dot product computed from the reference (the "F" entries of _stack_layer_cases), E_torch the distance of the same layer
composed from plain torch fp32 operations on the same inputs, measured here.  Every comparison prints
`[entry] case quantity: kernel <d> torch <d> F <absolute> bound <b> ratio <d / b>` with the distances in units of F.  Copies and
exact zeros (dbias, g_p under a zero mask, the dW column of a dead channel, untouched memory) are compared for equality."""
import contextlib
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stack_layer_cases as L  # noqa: E402
import _train_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu
f64 = torch.float64
DEV = "cuda"
_ci = ctypes.c_int


def _ts():
    from hotrack_amd import train_stack
    return train_stack


def _ok(rc, what):
    from hotrack_amd import pointnet2_hip
    pointnet2_hip._check(rc, what)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _poison(*shape, dtype=torch.float32):
    """0xFF bytes: NaN as float32, -1 as int32."""
    n = 1
    for s in shape:
        n *= s
    return torch.full((n * 4,), 255, dtype=torch.uint8, device=DEV).view(dtype).view(*shape)


def _untouched(t):
    return bool((t.contiguous().view(torch.int32) == -1).all())


def _padded(t, pad, off=0):
    """t (r, c) as columns [off, off + c) of a NaN-filled (r, c + pad) device buffer; returns the view."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device=DEV) if t.dtype == torch.float32 else \
        torch.full((t.shape[0], t.shape[1] + pad), -1, dtype=t.dtype, device=DEV)
    buf[:, off:off + t.shape[1]] = t.to(DEV)
    return buf[:, off:off + t.shape[1]]


def _copies(parts, ld):
    """(REP, 2 c) float64 parts -> the (REP, 2, ld) accumulator layout on the device."""
    c = parts.shape[1] // 2
    out = torch.zeros(L.REP, 2, ld, dtype=f64)
    out[:, 0, :c], out[:, 1, :c] = parts[:, :c], parts[:, c:]
    return out.reshape(-1).to(DEV)


def _total(sums, c):
    return sums.view(L.REP, 2, c).sum(0).reshape(-1)


def _check(entry, case, name, got, want, tor, F):
    dk, dt = T.dist(got, want, 0.0, F), T.dist(tor, want, 0.0, F)
    b = T.bound(dt)
    fmax = float(F.max()) if torch.is_tensor(F) else float(F)
    print(f"[{entry}] {case} {name}: kernel {dk:.3g} torch {dt:.3g} F {fmax:.3g} bound {b:.3g} ratio {dk / b:.3g}")
    assert dk <= b, (entry, case, name, dk, dt, fmax)


# ---- forward ------------------------------------------------------------------------------------------------------------------------
_FWD = {}


def _fwd_case(rows, k, n):
    """The case, its float64 reference and the fp32 torch composition: built once, shared, never modified."""
    key = (rows, k, n)
    if key not in _FWD:
        c = L.forward_case(rows, k, n, seed=7 * rows + 3 * k + n)
        x, w = c["x"].to(DEV), c["w"].to(DEV)
        ga, be, m = c["gamma"].to(DEV), c["beta"].to(DEV), L.MOMENTUM
        # the statistics from the SAME sums the kernel is given, rounded to float32, then float32 arithmetic throughout
        s32 = c["sums_in"].float().to(DEV)
        mean = s32[:k] / rows
        var = (s32[k:] / rows - mean * mean).clamp_min(0.0)
        invstd = 1.0 / torch.sqrt(var + L.EPS)
        y = torch.relu((x - mean) * invstd * ga + be) @ w.t()
        c["torch"] = {"mean": mean, "invstd": invstd, "y": y, "sums_out": torch.cat([y.sum(0), (y * y).sum(0)]),
                      "running_mean": (1 - m) * c["running_mean"].to(DEV) + m * (mean + c["conv_bias"].to(DEV)),
                      "running_var": (1 - m) * c["running_var"].to(DEV) + m * (var * (rows / (rows - 1.0)) if rows > 1 else var)}
        x64 = c["x"].double()
        c["parts"] = torch.stack([torch.cat([x64[r::L.REP].sum(0), (x64[r::L.REP] ** 2).sum(0)]) for r in range(L.REP)])
        _FWD[key] = c
    return _FWD[key]


class _FwdBufs:
    def __init__(self, c, padded):
        rows, k, n = c["rows"], c["k"], c["n"]
        px, pw, py, self.off = (4, 8, 8, 4) if padded else (0, 0, 0, 0)
        self.x, self.w = _padded(c["x"], px), _padded(c["w"], pw)
        self.ywide = _poison(rows, n + py)
        self.y = self.ywide[:, self.off:self.off + n]
        self.sums_in = _copies(c["parts"], k)
        self.gamma, self.beta, self.bias = c["gamma"].to(DEV), c["beta"].to(DEV), c["conv_bias"].to(DEV)
        self.rm, self.rv = c["running_mean"].to(DEV).clone(), c["running_var"].to(DEV).clone()
        self.nbt = torch.zeros((), dtype=torch.int64, device=DEV)
        self.save = _poison(2, k)
        self.sums_out = torch.zeros(2 * n * L.REP, dtype=f64, device=DEV)
        self.rows, self.k, self.n = rows, k, n

    def tg_fwd(self, sums=True):
        lib = _ts()._lib
        _ok(lib.pn2x_tg_fwd(self.rows, self.k, self.n, self.x.data_ptr(), self.x.stride(0), self.w.data_ptr(), self.w.stride(0),
                            self.y.data_ptr(), self.ywide.stride(0), self.sums_in.data_ptr(), self.gamma.data_ptr(), self.beta.data_ptr(),
                            self.bias.data_ptr(), L.EPS, L.MOMENTUM, self.rm.data_ptr(), self.rv.data_ptr(), self.nbt.data_ptr(),
                            self.save[0].data_ptr(), self.save[1].data_ptr(), self.sums_out.data_ptr() if sums else None, _st()), "tg_fwd")
        return self

    def record(self, sums=True):
        return _ts()._TgFwd2Problem(
            x=self.x.data_ptr(), w=self.w.data_ptr(), y=self.y.data_ptr(), sums_in=self.sums_in.data_ptr(), gamma=self.gamma.data_ptr(),
            beta=self.beta.data_ptr(), conv_bias=self.bias.data_ptr(), running_mean=self.rm.data_ptr(), running_var=self.rv.data_ptr(),
            num_batches_tracked=self.nbt.data_ptr(), save_mean=self.save[0].data_ptr(), save_invstd=self.save[1].data_ptr(),
            sums_out=self.sums_out.data_ptr() if sums else None, rows=self.rows, k=self.k, n=self.n, ldx=self.x.stride(0),
            ldw=self.w.stride(0), ldy=self.ywide.stride(0), eps=L.EPS, momentum=L.MOMENTUM)


def _fwd2(*bufs, sums=True):
    from hotrack_amd import train_ops
    _ok(_ts()._lib.pn2x_tg_fwd2(*train_ops._records(*(b.record(sums) for b in bufs)), _st()), "tg_fwd2")
    return bufs


def _check_forward(entry, case, c, b, sums=True):
    ref, tor, F = c["ref"], c["torch"], c["ref"]["F"]
    rows, k, n, m = c["rows"], c["k"], c["n"], L.MOMENTUM
    x64 = c["x"].double()
    _check(entry, case, "y", b.y, ref["y"], tor["y"], F["y"])
    # save_mean / save_invstd: float64 arithmetic on the sums (1e-15 of the terms), ONE rounding to float32
    _check(entry, case, "save_mean", b.save[0], ref["mean"], tor["mean"], 2 * L.U * ref["mean"].abs() + 1e-15 * x64.abs().mean(0) + 1e-30)
    _check(entry, case, "save_invstd", b.save[1], ref["invstd"], tor["invstd"], 4 * L.U * ref["invstd"])
    # running statistics: the float32 batch value (+ bias), two products and a sum in float32
    ub = ref["var"] * (rows / (rows - 1.0)) if rows > 1 else ref["var"]
    _check(entry, case, "running_mean", b.rm, ref["running_mean"], tor["running_mean"],
           4 * L.U * ((1 - m) * c["running_mean"].double().abs() + m * (ref["mean"].abs() + c["conv_bias"].double().abs())) + 1e-30)
    _check(entry, case, "running_var", b.rv, ref["running_var"], tor["running_var"],
           4 * L.U * ((1 - m) * c["running_var"].double().abs() + m * ub) + 1e-30)
    assert int(b.nbt) == ref["num_batches_tracked"]
    if b.off:   # the neighbouring columns of the wider buffer keep their sentinel
        assert _untouched(b.ywide[:, :b.off]) and _untouched(b.ywide[:, b.off + n:])
    if sums:
        got = _total(b.sums_out, n)
        y64 = b.y.double()
        own = torch.cat([y64.sum(0), (y64 * y64).sum(0)])
        # tight: a lane adds at most 16 values of a tile in float32 and (at these sizes) owns one tile, one more add joins two
        # lanes, everything above is float64 -- <= 17 u sum |terms|, taken with a factor two
        tight = 32 * L.U * torch.cat([y64.abs().sum(0), (y64 * y64).sum(0)]) + 1e-30
        d = T.dist(got, own, 0.0, tight)
        print(f"[{entry}] {case} sums_out vs own y: {d:.3g} (units of 32 u sum |terms|)")
        assert d <= 1.0, (entry, case, d)
        _check(entry, case, "sum_y", got[:n], ref["sums_out"][:n], tor["sums_out"][:n], F["sum_y"])
        _check(entry, case, "sum_y2", got[n:], ref["sums_out"][n:], tor["sums_out"][n:], F["sum_y2"])
    else:
        assert float(b.sums_out.abs().max()) == 0.0


@pytest.mark.parametrize("rows,k,n,padded", L.FWD_CASES)
def test_tg_fwd_matches_fp64(rows, k, n, padded):
    c = _fwd_case(rows, k, n)
    assert _ts()._lib.pn2x_tg_supported(k, n)
    _check_forward("tg_fwd", f"rows={rows} k={k} n={n} padded={padded}", c, _FwdBufs(c, padded).tg_fwd())


def test_tg_fwd2_supported_set():
    lib = _ts()._lib
    assert [(k, n) for k in L.FWD2_K for n in L.FWD2_N if lib.pn2x_tg_fwd2_supported(k, n)] == L.FWD2_SUPPORTED


@pytest.mark.parametrize("k,n", L.FWD2_SUPPORTED)
def test_tg_fwd2_matches_fp64(k, n):
    """Every accepted shape at every row count, padded and as a column block; the same inputs through pn2x_tg_fwd, which accepts
    all of these shapes too.  The last row count also runs with sums_out = NULL."""
    lib = _ts()._lib
    assert lib.pn2x_tg_fwd2_supported(k, n) and lib.pn2x_tg_supported(k, n)
    for rows in L.FWD2_ROWS:
        c = _fwd_case(rows, k, n)
        case = f"rows={rows} k={k} n={n}"
        (b,) = _fwd2(_FwdBufs(c, True))
        _check_forward("tg_fwd2", case, c, b)
        _check_forward("tg_fwd", case + " (fwd2 shape)", c, _FwdBufs(c, rows % 2 == 1).tg_fwd())
    (b,) = _fwd2(_FwdBufs(c, False), sums=False)
    _check_forward("tg_fwd2", case + " sums_out=NULL", c, b, sums=False)
    _check_forward("tg_fwd", case + " sums_out=NULL", c, _FwdBufs(c, False).tg_fwd(sums=False), sums=False)


def _same_forward(a, b, n):
    for x, y in ((a.ywide, b.ywide), (a.save, b.save), (a.rm, b.rm), (a.rv, b.rv), (a.nbt, b.nbt)):
        assert torch.equal(x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x,
                           y.contiguous().view(torch.int32) if y.dtype == torch.float32 else y)
    sa, sb = _total(a.sums_out, n), _total(b.sums_out, n)   # fp64 atomics: the order of the adds is free
    y64 = a.y.double()
    assert T.dist(sa, sb, 0.0, 1e-13 * torch.cat([y64.abs().sum(0), (y64 * y64).sum(0)]) + 1e-300) <= 1.0


@pytest.mark.parametrize("k,n,rows_a,rows_b", L.FWD2_PAIRS)
def test_tg_fwd2_pair_launch_is_two_single_launches(k, n, rows_a, rows_b):
    assert _ts()._lib.pn2x_tg_fwd2_pair_supported(k, n)
    ca, cb = _fwd_case(rows_a, k, n), _fwd_case(rows_b, k, n)
    pa, pb = _fwd2(_FwdBufs(ca, True), _FwdBufs(cb, False))
    (sa,), (sb,) = _fwd2(_FwdBufs(ca, True)), _fwd2(_FwdBufs(cb, False))
    _same_forward(pa, sa, n)
    _same_forward(pb, sb, n)
    _check_forward("tg_fwd2 pair", f"rows={rows_a}|{rows_b} k={k} n={n} [a]", ca, pa)
    _check_forward("tg_fwd2 pair", f"rows={rows_a}|{rows_b} k={k} n={n} [b]", cb, pb)


# ---- backward -----------------------------------------------------------------------------------------------------------------------
_TORCH_BWD = {}


def _torch_backward(c):
    """The layer's backward from plain torch fp32 operations on the same inputs (the given sums rounded to float32)."""
    key = id(c)
    if key in _TORCH_BWD:
        return _TORCH_BWD[key]
    d = lambda name: c[name].to(DEV)
    rows, n, gmode, kmax = c["rows"], c["n"], c["gmode"], c["kmax"]
    xi = (d("yi") - d("mean_i")) * d("invstd_i")
    pre_i = xi * d("gamma_i") + d("beta_i")
    zero = torch.zeros((), device=DEV)
    if gmode == 0:
        g = d("gsrc")
    elif gmode == 1:
        g = torch.where(pre_i > 0, d("gsrc"), zero)
    else:
        g = torch.zeros(rows // kmax, kmax, n, device=DEV)
        g.scatter_(1, d("arg").long().unsqueeze(1), d("gsrc").unsqueeze(1))
        g = torch.where(pre_i > 0, g.view(rows, n), zero)
    s = c["ref"]["own_sums"].float().to(DEV)
    dy = d("gamma_i") * d("invstd_i") * (g - s[:n] / rows - xi * (s[n:] / rows))
    xp = (d("yp") - d("mean_p")) * d("invstd_p")
    pre_p = xp * d("gamma_p") + d("beta_p")
    gp = torch.where(pre_p > 0, dy @ d("w"), zero)
    res = {"gp": gp, "sums_bwd_p": torch.cat([gp.sum(0), (gp * xp).sum(0)]), "dw": dy.t() @ torch.relu(pre_p), "dgamma": s[n:], "dbeta": s[:n]}
    _TORCH_BWD[key] = res
    return res


class _BwdBufs:
    """Device buffers of one layer's backward.  pad: extra floats per row of yi, yp, gp, w; wide_g: g is a column block (offset
    wide_g / 2) of a gradient wide_g columns wider while arg stays contiguous."""

    def __init__(self, c, pad=(0, 0, 0, 0), wide_g=0, start=0.0):
        self.c, rows, k, n = c, c["rows"], c["k"], c["n"]
        self.g = _padded(c["gsrc"], wide_g, wide_g // 2)
        self.arg = c["arg"].to(DEV).contiguous() if c["arg"] is not None else None
        self.yi, self.yp, self.w = _padded(c["yi"], pad[0]), _padded(c["yp"], pad[1]), _padded(c["w"], pad[3])
        self.gpwide = _poison(rows, k + pad[2])
        self.gp = self.gpwide[:, :k]
        for name in ("mean_i", "invstd_i", "gamma_i", "beta_i", "mean_p", "invstd_p", "gamma_p", "beta_p"):
            setattr(self, name, c[name].to(DEV))
        self.sums_i = _copies(c["sums_parts"], n)
        self.sums_p = torch.full((2 * k * L.REP,), start, dtype=f64, device=DEV)   # accumulated into: zeros, as the header requires
        self.dw, self.dgamma, self.dbeta, self.dbias = _poison(n, k), _poison(n), _poison(n), _poison(n)
        self.partials, self.reported = [], []

    def record(self, off=0, wd=None, raw_out=0, g_add=False):
        c, TS = self.c, _ts()
        k, n, gmode = c["k"], c["n"], c["gmode"]
        wd = n if wd is None else wd
        o4 = 4 * off
        np_ = int(TS._lib.pn2x_tg_bwd_partials(c["rows"], wd, k))
        assert np_ >= 1
        partial = _poison(np_ * wd * k)
        self.partials.append((partial, off, wd, np_))
        return TS._TgBwdSliceProblem(
            g=self.g.data_ptr() + o4, arg=(self.arg.data_ptr() + o4) if gmode == 2 else None, yi=self.yi.data_ptr() + o4,
            mean_i=self.mean_i.data_ptr() + o4, invstd_i=self.invstd_i.data_ptr() + o4, gamma_i=self.gamma_i.data_ptr() + o4,
            beta_i=self.beta_i.data_ptr() + o4, sums_bwd_i=self.sums_i.data_ptr() + 8 * off, w=self.w.data_ptr() + o4 * self.w.stride(0),
            yp=self.yp.data_ptr(), mean_p=self.mean_p.data_ptr(), invstd_p=self.invstd_p.data_ptr(), gamma_p=self.gamma_p.data_ptr(),
            beta_p=self.beta_p.data_ptr(), gp=self.gp.data_ptr(), sums_bwd_p=self.sums_p.data_ptr(), partial=partial.data_ptr(),
            dw=self.dw.data_ptr() + o4 * k, g_add=self.gp.data_ptr() if g_add else None, rows=c["rows"], partial_floats=partial.numel(),
            n=wd, k=k, gmode=gmode, ldg=self.g.stride(0), ldarg=n if gmode == 2 else 4, kmax=c["kmax"], ldyi=self.yi.stride(0), sums_ld=n,
            ldw=self.w.stride(0), ldyp=self.yp.stride(0), ldgp=self.gpwide.stride(0), ldga=self.gpwide.stride(0), raw_out=raw_out)

    def reduce(self, counts=None):
        """pn2x_tg_reduce_multi over exactly the reported partial tiles of every slice recorded so far."""
        c, lib = self.c, _ts()._lib
        k, n, m = c["k"], c["n"], len(self.partials)
        counts = counts if counts is not None else self.reported
        vp = lambda: (ctypes.c_void_p * m)()
        part, dw, sm, dg, db, dbi = vp(), vp(), vp(), vp(), vp(), vp()
        P, numel, ch, sld = (_ci * m)(), (_ci * m)(), (_ci * m)(), (_ci * m)()
        for j, ((partial, off, wd, np_), cnt) in enumerate(zip(self.partials, counts)):
            assert 1 <= cnt <= np_
            part[j], dw[j], sm[j] = partial.data_ptr(), self.dw.data_ptr() + 4 * off * k, self.sums_i.data_ptr() + 8 * off
            dg[j], db[j], dbi[j] = self.dgamma.data_ptr() + 4 * off, self.dbeta.data_ptr() + 4 * off, self.dbias.data_ptr() + 4 * off
            P[j], numel[j], ch[j], sld[j] = cnt, wd * k, wd, n
        _ok(lib.pn2x_tg_reduce_multi(m, part, P, numel, dw, sm, ch, sld if m > 1 or n != self.partials[0][2] else None, dg, db, dbi, _st()),
            "tg_reduce_multi")
        return self

    def launch(self, rec):
        from hotrack_amd import train_ops
        out = (_ci * 2)(0, 0)
        _ok(_ts()._lib.pn2x_tg_bwd_slice(*train_ops._records(rec), out, _st()), "tg_bwd_slice")
        self.reported.append(int(out[0]))
        return self

    def whole(self):
        self.launch(self.record()).reduce()
        self.keep = self.partials[0][0][:self.reported[0] * self.c["n"] * self.c["k"]]   # the partial tiles that were written
        return self


@contextlib.contextmanager
def _variant(v):
    lib = _ts()._lib
    _ok(lib.pn2x_tg_bwd_set_variant(v), "tg_bwd_set_variant")
    try:
        yield
    finally:
        _ok(lib.pn2x_tg_bwd_set_variant(1), "tg_bwd_set_variant")


def _check_backward(entry, case, b, weights=True):
    c = b.c
    ref, tor, F, k, n = c["ref"], _torch_backward(c), c["ref"]["F"], c["k"], c["n"]
    _check(entry, case, "g_p", b.gp, ref["gp"], tor["gp"], F["gp"])
    assert float((b.gp * (~ref["mask_p"]).to(DEV)).abs().max()) == 0.0       # exact zeros under the mask of layer p
    if b.gpwide.shape[1] > k:
        assert _untouched(b.gpwide[:, k:])
    got = _total(b.sums_p, k)
    _check(entry, case, "sum_g_p", got[:k], ref["sums_bwd_p"][:k], tor["sums_bwd_p"][:k], F["sum_g"])
    _check(entry, case, "sum_g_p_xhat", got[k:], ref["sums_bwd_p"][k:], tor["sums_bwd_p"][k:], F["sum_gx"])
    assert float(got[L.DEAD]) == 0.0 and float(got[k + L.DEAD]) == 0.0
    if weights:
        _check(entry, case, "dW", b.dw, ref["dw"], tor["dw"], F["dw"])
        assert float(b.dw[:, L.DEAD].abs().max()) == 0.0                      # the dead channel of layer p
        _check(entry, case, "dgamma", b.dgamma, ref["dgamma"], tor["dgamma"], F["dgamma"])
        _check(entry, case, "dbeta", b.dbeta, ref["dbeta"], tor["dbeta"], F["dbeta"])
        assert float(b.dbias.abs().max()) == 0.0


def test_tg_bwd_supported_set():
    lib = _ts()._lib
    widths = range(32, 513, 32)
    assert [(k, n) for k in widths for n in widths if lib.pn2x_tg_bwd_supported(k, n)] == sorted(L.BWD_SHAPES)
    assert [s for s in L.BWD_SHAPES if lib.pn2x_tg_bwd_pair_supported(*s)] == L.PAIR_SHAPES
    assert not lib.pn2x_tg_bwd_pair_supported(*L.PAIR_NO_KERNEL)


@pytest.mark.parametrize("gmode", [0, 1, 2])
@pytest.mark.parametrize("k,n", L.BWD_SHAPES)
def test_tg_bwd_slice_matches_fp64(k, n, gmode):
    for rows in L.BWD_ROWS:
        c = L.cached_backward_case(rows, k, n, gmode, rows if gmode == 2 else 1)
        for v in (1, 0):
            with _variant(v):
                b = _BwdBufs(c).whole()
            kernel = "tg_bwd2" if v == 1 and (k, n) in L.BWD2_SHAPES else "tg_bwd"
            _check_backward(f"tg_bwd_slice {kernel}", f"rows={rows} k={k} n={n} gmode={gmode} variant={v}", b)


def _persistent_rows(k, n):
    """One tile and a ragged tail more than the row count at which pn2x_tg_bwd_partials stops rising: the persistent loop runs a
    second round on one workgroup and ends on a ragged tile."""
    lib = _ts()._lib
    ks_w = int(lib.pn2x_tg_bwd_partials(1, n, k))       # one tile: one workgroup, ks_w partial tiles
    tiles = 1
    while tiles < 4096 and lib.pn2x_tg_bwd_partials(64 * (tiles + 1), n, k) > lib.pn2x_tg_bwd_partials(64 * tiles, n, k):
        tiles += 1
    assert tiles < 4096 and lib.pn2x_tg_bwd_partials(64 * tiles, n, k) == tiles * ks_w
    return 64 * (tiles + 1) + 17


@pytest.mark.parametrize("name", list(L.BWD_REDUCED))
def test_tg_bwd_slice_reduced_set(name):
    rows, gmode, kmax, opt = L.BWD_REDUCED[name]
    k, n = L.BWD_LARGEST
    for v in (1, 0):
        with _variant(v):
            if opt.get("persistent"):
                rows = _persistent_rows(k, n)
                assert int(_ts()._lib.pn2x_tg_bwd_partials(rows, n, k)) < (rows + 63) // 64
            c = L.cached_backward_case(rows, k, n, gmode, kmax)
            if opt.get("persistent"):   # built at this machine's row count: the builder's claims, checked here and not on the CPU
                for pre, moved, y in ((c["ref"]["pre_i"], c["moved"][0], c["yi"]), (c["ref"]["pre_p"], c["moved"][1], c["yp"])):
                    assert float(pre.abs().min()) >= L.MASK_MARGIN and moved <= 0.01 * y.numel()
                assert float(c["ref"]["xhat_i"].abs().max()) <= L.XHAT_MAX and float(c["ref"]["xhat_p"].abs().max()) <= L.XHAT_MAX
            b = _BwdBufs(c, pad=opt.get("pad", (0, 0, 0, 0)), wide_g=opt.get("wide_g", 0)).whole()
        _check_backward(f"tg_bwd_slice {'tg_bwd2' if v else 'tg_bwd'}", f"{name} rows={rows} k={k} n={n} gmode={gmode} kmax={kmax} variant={v}", b)


@pytest.mark.parametrize("k,n,wd,rows,gmode,kmax", L.CHAIN_CASES)
def test_tg_bwd_slice_chain_matches_whole_layer(k, n, wd, rows, gmode, kmax):
    """A layer wider than any instantiated kernel as consecutive column slices: raw_out = 1 on all but the last, g_add aliasing gp
    from the second on, sums_ld = the whole width; against the whole-layer reference."""
    c = L.cached_backward_case(rows, k, n, gmode, kmax)
    assert not _ts()._lib.pn2x_tg_bwd_supported(k, n) and _ts()._lib.pn2x_tg_bwd_supported(k, wd)
    for v in (1, 0):
        with _variant(v):
            b = _BwdBufs(c)
            nsl = n // wd
            for j in range(nsl):
                b.launch(b.record(off=j * wd, wd=wd, raw_out=1 if j + 1 < nsl else 0, g_add=j > 0))
                assert _untouched(b.dw[(j + 1) * wd:])                      # later slices' rows of dW: not yet touched
                assert float(b.dw[:(j + 1) * wd].abs().max()) == 0.0         # this slice's rows: zeroed for the reduction
                if j + 1 < nsl:
                    assert float(b.sums_p.abs().max()) == 0.0                # the sums of layer p wait for the last slice
                    # raw_out: gp holds the UNMASKED product of the slices so far (within the floor of the whole product),
                    # also where the mask of layer p is 0
                    hi = (j + 1) * wd
                    raw = c["ref"]["dy"][:, :hi] @ c["w"].double()[:hi]
                    d = T.dist(b.gp, raw, 0.0, c["ref"]["F"]["gp"])
                    print(f"[tg_bwd_slice chain] rows={rows} n={n} slice {j} variant={v} raw g_p: kernel {d:.3g} (units of F)")
                    assert d <= 1.0 and float((b.gp * (~c["ref"]["mask_p"]).to(DEV)).abs().max()) > 0.0
            b.reduce()
        _check_backward(f"tg_bwd_slice chain {'tg_bwd2' if v else 'tg_bwd'}", f"rows={rows} k={k} n={n}={nsl}x{wd} gmode={gmode} kmax={kmax} variant={v}", b)


def _pair_cases(k, n, gmode):
    return [L.cached_backward_case(rows, k, n, gmode, (1 if rows == 1 else 16) if gmode == 2 else 1) for rows in L.PAIR_ROWS]


def _launch_pair(ba, bb):
    from hotrack_amd import train_ops
    out = (_ci * 2)(0, 0)
    _ok(_ts()._lib.pn2x_tg_bwd_slice(*train_ops._records(ba.record(), bb.record()), out, _st()), "tg_bwd_slice pair")
    for b, cnt in zip((ba, bb), out):
        b.reported.append(int(cnt))
        b.reduce()


def _same_backward(a, b):
    for x, y in ((a.gpwide, b.gpwide), (a.dw, b.dw), (a.dgamma, b.dgamma), (a.dbeta, b.dbeta), (a.dbias, b.dbias)):
        assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
    k = a.c["k"]
    gp = a.c["ref"]["gp"]
    floor = 1e-13 * torch.cat([gp.abs().sum(0), (gp * a.c["ref"]["xhat_p"]).abs().sum(0)]).to(DEV) + 1e-300   # fp64 atomics in any order
    assert T.dist(_total(a.sums_p, k), _total(b.sums_p, k), 0.0, floor) <= 1.0


@pytest.mark.parametrize("gmode", [0, 1, 2])
@pytest.mark.parametrize("k,n", L.PAIR_SHAPES + [L.PAIR_NO_KERNEL])
def test_tg_bwd_slice_pair_launch_is_two_single_launches(k, n, gmode):
    """One row against 208, both orders, both variants.  128 -> 192 with a dense source (gmode 0 / 1) under variant 1 has no pair
    form of the register-resident-W kernel: the entry runs the pair on the round-4 kernel, so there the two single launches it must
    equal are the round-4 ones (variant 0) -- and it must meet the bound like every other combination."""
    small, big = _pair_cases(k, n, gmode)
    for v in (1, 0):
        fallback = v == 1 and (k, n) == (128, 192) and gmode != 2
        for ca, cb in ((small, big), (big, small)):
            with _variant(v):
                pa, pb = _BwdBufs(ca), _BwdBufs(cb)
                _launch_pair(pa, pb)
            with _variant(0 if fallback else v):
                sa, sb = _BwdBufs(ca).whole(), _BwdBufs(cb).whole()
            _same_backward(pa, sa)
            _same_backward(pb, sb)
            case = f"rows={ca['rows']}|{cb['rows']} k={k} n={n} gmode={gmode} variant={v}{' (round-4 pair kernel)' if fallback else ''}"
            _check_backward("tg_bwd_slice pair", case + " [a]", pa)
            _check_backward("tg_bwd_slice pair", case + " [b]", pb)


# ---- the two-kernel route -----------------------------------------------------------------------------------------------------------
def _two_kernel(c, deferred, start=0.0):
    lib = _ts()._lib
    b = _BwdBufs(c, start=start)
    rows, k, n, gmode = c["rows"], c["k"], c["n"], c["gmode"]
    dy = (gmode, b.g.data_ptr(), b.g.stride(0), b.arg.data_ptr() if gmode == 2 else None, c["kmax"], b.yi.data_ptr(), b.yi.stride(0),
          b.mean_i.data_ptr(), b.invstd_i.data_ptr(), b.gamma_i.data_ptr(), b.beta_i.data_ptr(), b.sums_i.data_ptr())
    stats_p = (b.mean_p.data_ptr(), b.invstd_p.data_ptr(), b.gamma_p.data_ptr(), b.beta_p.data_ptr())
    _ok(lib.pn2x_tg_dgrad(rows, n, k, *dy, b.w.data_ptr(), b.w.stride(0), b.yp.data_ptr(), b.yp.stride(0), *stats_p, b.gp.data_ptr(),
                          b.gpwide.stride(0), b.sums_p.data_ptr(), _st()), "tg_dgrad")
    pf = int(lib.pn2x_tg_wgrad_partial_floats(rows, n, k))
    assert pf >= n * k
    partial, cnt = _poison(pf), _ci(0)
    _ok(lib.pn2x_tg_wgrad(rows, n, k, *dy, b.yp.data_ptr(), b.yp.stride(0), *stats_p, partial.data_ptr(), pf, b.dw.data_ptr(),
                          b.dgamma.data_ptr(), b.dbeta.data_ptr(), b.dbias.data_ptr(), ctypes.byref(cnt) if deferred else None, _st()), "tg_wgrad")
    if deferred:
        assert 1 <= cnt.value <= pf // (n * k)
        assert float(b.dw.abs().max()) == 0.0     # zeroed, waiting for the reduction
        b.partials.append((partial, 0, n, cnt.value))
        b.reduce(counts=[cnt.value])
        b.keep = partial[:cnt.value * n * k]
    return b


@pytest.mark.parametrize("gmode", [0, 1, 2])
@pytest.mark.parametrize("kd,n", L.TWO_KERNEL_SHAPES)
def test_tg_dgrad_wgrad_match_fp64(kd, n, gmode):
    """(kd, n) = (channels of layer i, channels of layer p), pn2x_tg_dgrad's names; the reference's (k, n) = (n, kd).  The routed
    source takes row counts that are multiples of kmax next to the same tile edges (_stack_layer_cases.TWO_KERNEL_ROUTED).
    The immediate reduction (n_partials = NULL) and the deferred one must give the same bits: 32 -> 32 at 544 / 545 / 552 rows
    writes 68 - 72 partial tiles, where a reduction kernel of the immediate path's own once cut them into two slices and the
    deferred one into one."""
    lib = _ts()._lib
    assert lib.pn2x_tg_supported(kd, n) and lib.pn2x_tg_supported(n, kd) and n % 32 == 0
    runs = L.TWO_KERNEL_ROUTED if gmode == 2 else [(rows, 1) for rows in L.TWO_KERNEL_ROWS]
    for rows, kmax in runs:
        c = L.cached_backward_case(rows, n, kd, gmode, kmax)
        now, later = _two_kernel(c, False), _two_kernel(c, True)
        case = f"rows={rows} kd={kd} n={n} gmode={gmode} kmax={kmax}"
        _check_backward("tg_dgrad/tg_wgrad immediate", case, now)
        _check_backward("tg_dgrad/tg_wgrad deferred", case, later)
        _same_backward(now, later)


# ---- repeatability ------------------------------------------------------------------------------------------------------------------
def test_forward_entries_repeat_bitwise_and_accumulate_sums():
    for entry, k, n, rows in (("tg_fwd", 96, 192, 129), ("tg_fwd2", 128, 192, 64 * 5 + 17)):
        c = _fwd_case(rows, k, n)
        run = (lambda b: b.tg_fwd()) if entry == "tg_fwd" else (lambda b: _fwd2(b)[0])
        a, b = run(_FwdBufs(c, True)), run(_FwdBufs(c, True))
        _same_forward(a, b, n)
        # sums_out accumulates: from a non-zero start the result is that start plus the sums, to float64 rounding
        d = _FwdBufs(c, True)
        d.sums_out.fill_(3.0)
        run(d)
        y64 = a.y.double()
        floor = 1e-13 * (torch.cat([y64.abs().sum(0), (y64 * y64).sum(0)]) + 3.0 * L.REP)
        assert T.dist(_total(d.sums_out, n), _total(a.sums_out, n) + 3.0 * L.REP, 0.0, floor) <= 1.0, entry


def test_backward_entries_repeat_bitwise_and_accumulate_sums():
    k, n = L.BWD_LARGEST
    c = L.cached_backward_case(208, k, n, 2, 16)
    c2 = L.cached_backward_case(129, 128, 192, 1, 1)
    runs = [("tg_bwd_slice", lambda start: _BwdBufs(c, start=start).whole()),
            ("tg_dgrad/tg_wgrad", lambda start: _two_kernel(c2, True, start=start))]
    for entry, run in runs:
        a, b = run(0.0), run(0.0)
        _same_backward(a, b)
        assert torch.equal(a.keep.view(torch.int32), b.keep.view(torch.int32)), entry    # the partial tiles, bit for bit
        d = run(3.0)
        kk = a.c["k"]
        gp = a.c["ref"]["gp"]
        floor = 1e-13 * (torch.cat([gp.abs().sum(0), (gp * a.c["ref"]["xhat_p"]).abs().sum(0)]).to(DEV) + 3.0 * L.REP)
        assert T.dist(_total(d.sums_p, kk), _total(a.sums_p, kk) + 3.0 * L.REP, 0.0, floor) <= 1.0, entry
