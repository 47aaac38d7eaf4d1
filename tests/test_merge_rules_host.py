"""The fused merge's argument rules are written once (csrc/hm_merge_rules.h) and compiled into both builds of the C ABI. This sweep holds the
two builds to it: a call that is valid for hm_merge, hm_merge_std_table and hm_merge_std_f32 (7 uint8 frames of 64 x 64 x 3 with dark maps, a
flat field and all three outputs), its float64-frame twin, and every single fault applied to them, through `_describe` and
`_algorithmic_bytes` of each entry on libhdrmerge.so (dry: nothing is launched) and libhdrmerge_host.so. No GPU needed.

Status and byte count must agree between the builds for every case. The one exception is the documented difference between the builds: a
table call with more than HM_MAX_FRAMES frames or variant <= -2 is HM_EUNSUPPORTED on the device build and HM_OK on the host build.

tools/merge_rules_sweep.py prints the same sweep (with the describe strings) for comparing two commits."""
import ctypes as C

import pytest

pytest.importorskip("torch")

BASE = 1 << 20
NMAX = 33                                                      # every per-frame array has room for the largest n_frames of the sweep
ENTRIES = ("hm_merge", "hm_merge_std_table", "hm_merge_std_f32")


class Call:
    """One call of `entry` with fake, aligned pointers; perturbations edit `a` (the struct), `extra` (the entry's own pointer) and the
    per-frame arrays `fr`, `sd` (args->stds for hm_merge, stds_f32 for hm_merge_std_f32), `dk`, `ex` in place."""

    def __init__(self, entry, f64):
        from camera_linearity_amd import _native as nat
        self.entry, self.f64, self.null_args = entry, f64, False
        a = self.a = nat.MergeArgs()
        a.struct_size = C.sizeof(nat.MergeArgs)
        a.n_frames, a.channels, a.variant, a.out_kind = 7, 3, 0, nat.HM_OUT_F64
        a.height = a.rows = a.buf_rows = a.width = 64
        self.fr = (C.c_void_p * NMAX)(*[BASE * (i + 1) for i in range(NMAX)])
        if f64:
            a.frames_f64 = C.cast(self.fr, C.POINTER(C.c_void_p))
        else:
            a.frames_u8 = C.cast(self.fr, C.POINTER(C.c_void_p))
        self.ex = (C.c_double * NMAX)(*[1e-3 * 1.2 ** i for i in range(NMAX)])
        a.exposures = C.cast(self.ex, C.POINTER(C.c_double))
        a.icrf, a.w_lut, a.out_val = BASE * 40, BASE * 41, BASE * 42
        a.icrf_diff, a.dw_lut, a.out_std, a.out_sum_w = BASE * 43, BASE * 44, BASE * 45, BASE * 48
        a.flat_u8, a.flat_std = BASE * 46, BASE * 47
        self.dk = (C.c_void_p * NMAX)(*[BASE * 90] * NMAX)
        self.dm = (C.c_int32 * NMAX)(*[13] * NMAX)
        a.darks_u8 = C.cast(self.dk, C.POINTER(C.c_void_p))
        a.dark_min_dn = C.cast(self.dm, C.POINTER(C.c_int32))
        a.median_k = 3
        a.hot_workspace, a.hot_workspace_bytes = BASE * 91, nat.hip_lib.hm_merge_hot_workspace_bytes(64 * 64 * 3)
        self.sd, self.extra = None, None
        if entry != "hm_merge_std_table":
            self.sd = (C.c_void_p * NMAX)(*[BASE * (50 + i) for i in range(NMAX)])
        if entry == "hm_merge":
            a.stds = C.cast(self.sd, C.POINTER(C.c_void_p))
        elif entry == "hm_merge_std_table":
            self.extra = BASE * 49
        else:
            self.extra = C.addressof(self.sd)

    def probe(self, lib):
        """-> (status of _describe, the kernels it names, _algorithmic_bytes)"""
        buf = C.create_string_buffer(b"untouched", 1024)
        ref = None if self.null_args else C.byref(self.a)
        if self.entry == "hm_merge":
            rc = lib.hm_merge_describe(ref, buf, 1024)
        else:
            rc = getattr(lib, self.entry + "_describe")(ref, self.extra, C.addressof(buf), 1024)
        return rc, buf.value.decode(), getattr(lib, self.entry + "_algorithmic_bytes")(ref)


def _set(field, value):
    return lambda c: setattr(c.a, field, value)


def _shift(field, by):
    return lambda c: setattr(c.a, field, getattr(c.a, field) + by)


def _shift_all(array, by):
    def f(c):
        arr = getattr(c, array)
        for i in range(NMAX):
            arr[i] += by
    return f


def _entry_null(array, i):
    def f(c):
        getattr(c, array)[i] = None
    return f


def _tile(**kw):
    def f(c):
        for k, v in kw.items():
            setattr(c.a, k, v)
    return f


def _extra(value):
    return lambda c: setattr(c, "extra", value(c) if callable(value) else value)


def _null_args(c):
    c.null_args = True


POINTER_FIELDS = ("frames_u8", "frames_f64", "stds", "exposures", "icrf", "icrf_diff", "w_lut", "dw_lut", "darks_u8", "dark_min_dn", "flat_u8",
                  "flat_std", "out_val", "out_std", "out_sum_w", "hot_workspace")


def perturbations(entry, f64):
    """(name, function on a Call) of every single fault that applies to this entry and frame type; "base" is the unperturbed call."""
    frames = "frames_f64" if f64 else "frames_u8"
    p = [("base", lambda c: None), ("args=NULL", _null_args)]
    # each pointer field NULL in turn (the fields the base leaves NULL are skipped), each per-frame array with one NULL entry, the entry's own pointer
    for f in POINTER_FIELDS:
        if f in ("frames_u8", "frames_f64") and f != frames or f == "stds" and entry != "hm_merge":
            continue
        p.append((f + "=NULL", _set(f, None)))
    p += [("out_val=out_std=NULL", _tile(out_val=None, out_std=None)), ("frames[3]=NULL", _entry_null("fr", 3)), ("darks[2]=NULL", _entry_null("dk", 2))]
    if entry != "hm_merge_std_table":
        p.append(("stds[6]=NULL", _entry_null("sd", 6)))
    if entry != "hm_merge":
        p.append(("extra=NULL", _extra(None)))
    # misaligned by 2 and by 4 bytes: output pointers (float64 and float32 outputs), std pointers, the table, float64 frame pointers
    for by in (2, 4):
        for f in ("out_val", "out_std", "out_sum_w"):
            p.append((f"{f}+{by}", _shift(f, by)))
            p.append((f"{f}+{by},out_kind=1", lambda c, f=f, by=by: (_shift(f, by)(c), _set("out_kind", 1)(c))))
        if entry != "hm_merge_std_table":
            p.append((f"stds+{by}", _shift_all("sd", by)))
        else:
            p.append((f"table+{by}", _extra(lambda c, by=by: c.extra + by)))
        if f64:
            p.append((f"frames+{by}", _shift_all("fr", by)))
    p += [(f"n_frames={n}", _set("n_frames", n)) for n in (0, 1, 32, 33)]
    p += [(f"channels={ch}", _set("channels", ch)) for ch in (0, 4, 5)]
    p += [(f"rows=0,row0={r}", _tile(rows=0, row0=r)) for r in (10, 64, 65, -1)]                       # inside the image (and at its end), outside it
    p += [("halo<2,median_k=5", _tile(row0=8, rows=16, buf_row0=7, buf_rows=18, median_k=5)),
          ("halo=2,median_k=5", _tile(row0=8, rows=16, buf_row0=6, buf_rows=20, median_k=5))]
    p += [(f"median_k={k}", _set("median_k", k)) for k in (2, 4, 9)]
    p.append(("flat_u8+flat_f64", _set("flat_f64", BASE * 92)))
    p += [(f"out_kind={k}", _set("out_kind", k)) for k in (0, 1, 2)]
    p += [(f"variant={v}", _set("variant", v)) for v in (0, -1, -2, -3)]
    p += [(f"struct_size={s}", _set("struct_size", s)) for s in (100, 264, 280, 296)]
    p.append(("exposure[4]=0", lambda c: c.ex.__setitem__(4, 0.0)))
    return p


def cases():
    """-> (id, Call) of the whole sweep"""
    for entry in ENTRIES:
        for f64 in (False, True):
            for name, fn in perturbations(entry, f64):
                c = Call(entry, f64)
                fn(c)
                yield f"{entry}/{'f64' if f64 else 'u8'}/{name}", c


def device_only_refusal(c):
    """The one documented difference between the builds (hm_merge_rules.h). This list is part of the specification: it does not grow."""
    return c.entry == "hm_merge_std_table" and not c.null_args and (c.a.n_frames == 33 or c.a.variant <= -2)


def test_rules_agree_between_builds():
    from camera_linearity_amd import _native as nat
    hip, host = nat.hip_lib, nat.host_lib()
    seen, exceptions = set(), 0
    for cid, c in cases():
        d_rc, d_names, d_bytes = c.probe(hip)
        h_rc, h_names, h_bytes = c.probe(host)
        assert d_bytes == h_bytes, (cid, d_bytes, h_bytes)
        if device_only_refusal(c):
            assert (d_rc, h_rc) == (nat.HM_EUNSUPPORTED, nat.HM_OK), (cid, d_rc, h_rc)
            exceptions += 1
        else:
            assert d_rc == h_rc, (cid, d_rc, h_rc)
        for rc, names in ((d_rc, d_names), (h_rc, h_names)):
            assert (names not in ("", "untouched")) == (rc == nat.HM_OK and c.a.rows > 0), (cid, rc, names)   # kernels are named for calls that run, only
        seen.add(d_rc)
    assert exceptions == 2 * 3                                 # n_frames = 33, variant = -2, -3 on both frame types
    # the sweep reaches every status an argument can earn
    assert seen == {nat.HM_OK, nat.HM_EINVAL, nat.HM_ESHAPE, nat.HM_EALIGN, nat.HM_EUNSUPPORTED}


def test_base_calls_are_valid_for_all_three_entries():
    from camera_linearity_amd import _native as nat
    for entry in ENTRIES:
        for f64 in (False, True):
            for lib in (nat.hip_lib, nat.host_lib()):
                rc, names, nbytes = Call(entry, f64).probe(lib)
                assert rc == nat.HM_OK and names and nbytes > 0, (entry, f64, rc, names)
