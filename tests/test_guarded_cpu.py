"""The detector detects: tests/guarded.py on CPU tensors with fake operators written here (seeded defects live ONLY here, never in a
kernel), plus a static check that every allocation of the binding goes through a route the arena intercepts."""
import ast
import os
import struct
import types

import pytest
import torch

import guarded as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "custom-diffusion360_amd", "cd360")

# A fake binding module: like cd360/ops.py it allocates its outputs and workspaces itself, through the module-level name `torch`, and calls
# the "library" through load().  Every op is out[rows, cols] = 2 x with a one-element workspace holding cols; `defect` seeds one fault.
FAKE_SRC = '''
def scale2(x, defect=None):
    rows, cols = x.shape
    out = torch.empty(rows, cols, dtype=x.dtype, device=x.device)
    ws = torch.empty(8, dtype=torch.float32, device=x.device)
    acc = torch.zeros(rows, dtype=torch.float32, device=x.device)
    load().cd360_fake_scale2(x, out, ws, acc, defect)
    return out, acc


def make_full(device):
    return torch.full((4,), 1.0, device=device)


def make_ones(device):
    return torch.ones(4, device=device)


def make_strided(device):
    return torch.empty_strided((2, 2), (2, 1), device=device)
'''


def _beyond(t, offset_elems):
    """One element at `offset_elems` from t's first element, outside its bounds: what a kernel with a wrong bound does."""
    return t.as_strided((1,), (1,), t.storage_offset() + offset_elems)


class FakeLib:
    def cd360_fake_scale2(self, x, out, ws, acc, defect):
        rows, cols = x.shape
        ws[0] = float(cols)  # written before it is read
        n = rows - 1 if defect == "skip_last_row" else rows
        out[:n] = x[:n] * 2
        acc += x.float().sum(1) / ws[0] * cols  # acc arrives zeroed (torch.zeros): callers rely on it
        if defect == "write_past_out":
            _beyond(out, out.numel()).fill_(1.0)
        if defect == "write_before_out":
            _beyond(out, -1).fill_(1.0)
        if defect == "write_ws_guard":
            _beyond(ws, ws.numel() + 3).fill_(1.0)
        if defect == "read_unwritten_ws":
            out[0, 0] += ws[5]  # slot 5 was never written
        if defect == "modify_input":
            x[1, 2] += 1.0
        return 0

    def cd360_fake_other(self):
        return 0

    def not_an_entry_point(self):
        return 0


def fake_binding():
    m = types.ModuleType("fake_ops")
    lib = FakeLib()
    m.torch = torch
    m.load = lambda: lib
    exec(compile(FAKE_SRC, "fake_ops.py", "exec"), m.__dict__)
    return m, lib


def run(defect=None, declares=("cd360_fake_scale2",), dtype=torch.float32, **kw):
    m, lib = fake_binding()
    x = (torch.arange(5 * 7, dtype=torch.float32).reshape(5, 7) / 8).to(dtype)
    return _run_twice(m, lib, lambda x, guard=None: _with_lib(m, guard, lambda: m.scale2(x, defect)), (x,), declares, **kw)


def _with_lib(m, guard, body):
    """The fake module's load() returns the recorder of the running guard, as cd360._lib.load() does for the real binding."""
    saved = m.load
    m.load = lambda: guard.lib
    try:
        return body()
    finally:
        m.load = saved


def _run_twice(m, lib, fn, inputs, declares, **kw):
    fn.wants_guard = True
    return G.run_twice(fn, inputs, declares=declares, modules=[m], lib=lib, **kw)


# ---------------------------------------------------------------------------------------------------------------- P1 .. P4
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_correct_op_passes(dtype):
    (o1, a1), (o2, a2) = run(dtype=dtype)
    x = (torch.arange(35, dtype=torch.float32).reshape(5, 7) / 8).to(dtype)
    assert torch.equal(o1, x * 2) and torch.equal(o2, o1) and torch.equal(a1, x.float().sum(1))


@pytest.mark.parametrize("defect, side, first, last", [
    ("write_past_out", "back", 0, 3),       # one fp32 element behind the 5 x 7 output
    ("write_before_out", "front", -4, -1),  # one fp32 element in front of it
])
def test_stray_write_around_output_fails_p1(defect, side, first, last):
    with pytest.raises(G.GuardError, match=r"P1 stray write") as e:
        run(defect)
    msg = str(e.value)
    assert "fake_ops.py:4 in scale2" in msg and "shape (5, 7)" in msg and "torch.float32" in msg and "(empty)" in msg
    assert f"{side} guard damaged, bytes {first:+d} .. {last:+d}" in msg
    assert "fake_ops.py:5" not in msg and "fake_ops.py:6" not in msg  # only the damaged allocation is named


def test_stray_write_behind_workspace_fails_p1():
    with pytest.raises(G.GuardError, match=r"P1 stray write") as e:
        run("write_ws_guard")
    msg = str(e.value)
    assert "fake_ops.py:5 in scale2" in msg and "shape (8,)" in msg and "back guard damaged, bytes +12 .. +15" in msg
    assert "fake_ops.py:4" not in msg


def test_bf16_one_element_overrun_is_two_bytes():
    with pytest.raises(G.GuardError, match=r"back guard damaged, bytes \+0 \.\. \+1 ") as e:
        run("write_past_out", dtype=torch.bfloat16)
    assert "torch.bfloat16" in str(e.value)


def test_skipped_last_row_fails_p2():
    with pytest.raises(G.GuardError, match=r"P2 not fully written / uninitialised read: result\[0\].*7 non-finite elements.*flat index 28 \.\. 34"):
        run("skip_last_row")


def test_unwritten_workspace_read_fails_p2():
    with pytest.raises(G.GuardError, match=r"P2 not fully written / uninitialised read: result\[0\].*flat index 0 \.\. 0"):
        run("read_unwritten_ws")


def test_p2_bit_comparison_catches_what_finiteness_cannot():
    """int32 output with an unwritten tail: -1 under 0xFF is 'finite'; the 0x7F run differs."""
    m, lib = fake_binding()

    def fn(x, guard=None):
        out = m.torch.empty(6, dtype=torch.int32)
        out[:5] = x
        return out
    with pytest.raises(G.GuardError, match=r"P2 .*differs between the 0xFF and the 0x7F run in 1 elements, flat index 5 \.\. 5"):
        _run_twice(m, lib, fn, (torch.arange(5, dtype=torch.int32),), ())


def test_valid_region_exempts_only_what_it_leaves_out():
    m, lib = fake_binding()

    def fn(x, guard=None):
        out = m.torch.empty(2, 8)
        out[:, :5] = x  # columns 5 .. 7: pad the (fake) header leaves unspecified
        return out
    x = torch.ones(2, 5)
    _run_twice(m, lib, fn, (x,), (), valid=lambda r: r[:, :5])
    with pytest.raises(G.GuardError, match=r"P2 "):
        _run_twice(m, lib, fn, (x,), (), valid=lambda r: r[:, :6])


def test_modified_input_fails_p3():
    with pytest.raises(G.GuardError, match=r"P3 operand modified: input 0 .*shape \(5, 7\)"):
        run("modify_input")


def test_inout_argument_is_restored_and_compared():
    m, lib = fake_binding()

    def step(x, guard=None):  # in place, like cd360_cfg_euler_step_cl
        x += 1
    x = torch.zeros(4)
    _run_twice(m, lib, step, (x,), (), inout=(0,))
    assert torch.equal(x, torch.ones(4))  # the second run started from the saved state, not from the first run's result
    with pytest.raises(G.GuardError, match=r"P3 operand modified"):
        _run_twice(m, lib, step, (x,), ())


def test_undeclared_entry_point_fails_p4():
    with pytest.raises(G.GuardError, match=r"P4 entry point not called: .*\['cd360_fake_other'\].*saw \['cd360_fake_scale2'\]"):
        run(declares=("cd360_fake_scale2", "cd360_fake_other"))


def test_recorder_notes_calls_not_lookups():
    rec = G.Recorder(FakeLib())
    f = rec.cd360_fake_other
    assert rec.called == []
    f()
    rec.not_an_entry_point()
    assert rec.called == ["cd360_fake_other"]


def test_recorded_adds_a_second_library_to_the_guards_list_and_restores_load():
    """guarded.recorded on a fake module: calls through module.load() land in the guard's list next to the first library's; module.load
    is the module's own again after a normal exit and after the body raised, and returns the same library object as before."""
    m, lib = fake_binding()
    other, load = FakeLib(), m.load
    with G.guarded(G.Arena(0xFF), modules=[m], lib=other) as g:
        g.lib.cd360_fake_other()
        with G.recorded(g, m) as rec:
            assert m.load() is rec and m.load is not load
            m.load().cd360_fake_other()
            m.load().not_an_entry_point()
            m.scale2(torch.ones(2, 3))
        assert m.load is load and m.load() is lib
        assert g.lib.called == ["cd360_fake_other", "cd360_fake_other", "cd360_fake_scale2"]
        with pytest.raises(RuntimeError, match="boom"):
            with G.recorded(g, m):
                m.load().cd360_fake_other()
                raise RuntimeError("boom")
        assert m.load is load and m.load() is lib
        assert g.lib.called[3:] == ["cd360_fake_other"] and g.called == {"cd360_fake_other", "cd360_fake_scale2"}


# ---------------------------------------------------------------------------------------------------------------- arena / proxy
@pytest.mark.parametrize("poison", G.POISONS)
@pytest.mark.parametrize("shape, dtype", [((3, 5, 7), torch.bfloat16), ((1,), torch.float32), ((0,), torch.uint8), ((1000, 300), torch.float32),
                                          ((600000,), torch.bfloat16)])
def test_arena_layout(poison, shape, dtype):
    a = G.Arena(poison)
    p = G.TorchProxy(a)
    t = p.empty(*shape, dtype=dtype, device="cpu")
    z = p.zeros(shape, dtype=dtype)
    blk = a.blocks[0]
    assert t.shape == shape and t.dtype == dtype and t.is_contiguous() and z.shape == shape
    if t.numel():
        assert t.data_ptr() % 256 == 0 and z.data_ptr() % 256 == 0
        assert bool((t.view(-1).view(torch.uint8) == poison).all()) and bool((z.view(-1).view(torch.uint8) == 0).all())
    want = min(max(4096, (blk.nbytes + 255) // 256 * 256), 1 << 20)
    assert G.guard_bytes(blk.nbytes) == want and blk.front >= want and blk.raw.numel() - blk.front - blk.nbytes >= want
    assert bool((blk.raw[:blk.front] == 0xA5).all()) and bool((blk.raw[blk.front + blk.nbytes:] == 0xA5).all())
    a.check()


def test_poisons_read_as_documented():
    for poison, f32, i32 in ((0xFF, float("nan"), -1), (0x7F, struct.unpack("<f", b"\x7f" * 4)[0], 0x7F7F7F7F)):
        p = G.TorchProxy(G.Arena(poison))
        f, b, i = p.empty(2, dtype=torch.float32), p.empty(2, dtype=torch.bfloat16), p.empty(2, dtype=torch.int32)
        assert int(i[0]) == i32
        if poison == 0xFF:
            assert bool(f.isnan().all()) and bool(b.isnan().all())
        else:
            assert float(f[0]) == f32 and 3.38e38 < f32 < 3.40e38 and abs(float(b[0]) - 3.39e38) < 1e36 and bool(torch.isfinite(b).all())


def test_like_forms_follow_torch_layout():
    p = G.TorchProxy(G.Arena(0xFF))
    x = torch.zeros(4, 6, dtype=torch.bfloat16)
    for src in (x, x.t(), x[:, :3], x.reshape(2, 2, 6).permute(0, 2, 1)):
        for got, want in ((p.empty_like(src), torch.empty_like(src)), (p.zeros_like(src, dtype=torch.float32), torch.zeros_like(src, dtype=torch.float32))):
            assert got.shape == want.shape and got.stride() == want.stride() and got.dtype == want.dtype
    assert bool((p.zeros_like(x) == 0).all())
    assert p.float32 is torch.float32 and p.cat is torch.cat and p.nn is torch.nn  # everything else is torch's


@pytest.mark.parametrize("route", ["make_full", "make_ones", "make_strided"])
def test_proxy_refuses_unguarded_gpu_routes(route):
    m, lib = fake_binding()
    with G.guarded(G.Arena(0xFF), modules=[m], lib=lib):
        with pytest.raises(G.GuardError, match="allocation route on the GPU that the arena does not intercept"):
            getattr(m, route)("cuda")  # a device string only: the raise comes before anything touches a GPU
        with pytest.raises(G.GuardError):
            getattr(m, route)(torch.device("cuda", 0))
        assert getattr(m, route)("cpu").numel() == 4  # host tables pass through


def test_proxy_removed_after_exception():
    m, lib = fake_binding()
    with pytest.raises(RuntimeError, match="boom"):
        with G.guarded(G.Arena(0xFF), modules=[m], lib=lib) as g:
            assert m.torch is g.torch and isinstance(m.torch, G.TorchProxy)
            raise RuntimeError("boom")
    assert m.torch is torch


def test_real_binding_is_patched_and_restored():
    """guarded() on the package itself: the three modules see the proxy, cd360._lib.load is swapped for the recorder's, both come back."""
    import importlib
    mods = [importlib.import_module(n) for n in G.MODULES]
    L = importlib.import_module("cd360._lib")
    load = L.load
    sentinel = FakeLib()
    with pytest.raises(KeyError):
        with G.guarded(G.Arena(0x7F), lib=sentinel) as g:
            assert all(m.torch is g.torch for m in mods) and L.load() is g.lib and g.lib._lib is sentinel
            raise KeyError("out")
    assert all(m.torch is torch for m in mods) and L.load is load


# ---------------------------------------------------------------------------------------------------------------- the net stays closed
INTERCEPTED = {"empty", "empty_like", "zeros", "zeros_like"}
ALLOCATING = INTERCEPTED | {"ones", "ones_like", "full", "full_like", "empty_strided", "rand", "randn", "rand_like", "randn_like",
                            "new_empty", "new_zeros", "new_ones", "new_full", "new_empty_strided"}
# Tensor.new_* calls on host-side tables (never handed to a kernel as an output or a workspace): (file, line, call)
HOST_TABLE_ALLOCS = {
    ("nerf.py", 176, "new_zeros"),    # zero pad columns of the fp32 weight slice Wp, built once per weight set on the weights' device by torch.cat
    ("sampler.py", 47, "new_zeros"),  # the trailing 0 of the host-computed sigma schedule
}
PROXIED_FILES = ("ops.py", "nerf.py", "grad.py")


def _alloc_calls(fname):
    tree = ast.parse(open(os.path.join(PKG, fname)).read(), fname)
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in ALLOCATING:
            base = node.func.value
            yield node.lineno, node.func.attr, isinstance(base, ast.Name) and base.id == "torch"


def test_every_allocation_of_the_binding_is_intercepted():
    seen = 0
    for fname in PROXIED_FILES:
        for line, attr, on_torch in _alloc_calls(fname):
            seen += 1
            if on_torch and attr in INTERCEPTED:
                continue
            assert (fname, line, attr) in HOST_TABLE_ALLOCS, (
                f"cd360/{fname}:{line}: {'torch.' if on_torch else 'Tensor.'}{attr} allocates past the guarded arena (tests/guarded.py): use "
                "torch.empty / empty_like / zeros / zeros_like, or list a host-side table in HOST_TABLE_ALLOCS")
    assert seen >= 90  # ops.py alone holds 64 empty + 18 empty_like + 9 zeros: the scan found them
    for fname, line, attr in HOST_TABLE_ALLOCS:  # the list cannot rot: every entry still points at such a call
        assert any(l == line and a == attr and not t for l, a, t in _alloc_calls(fname)), (fname, line, attr)


def test_binding_modules_reach_torch_by_that_name_only():
    """The proxy replaces the module attribute `torch`: an `import torch as th` or `from torch import empty` would slip past it."""
    for fname in PROXIED_FILES:
        tree = ast.parse(open(os.path.join(PKG, fname)).read(), fname)
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                for a in node.names:
                    assert not (a.name == "torch" and a.asname not in (None, "torch")), (fname, node.lineno)
            if isinstance(node, ast.ImportFrom) and node.module == "torch":
                assert not {a.name for a in node.names} & ALLOCATING, (fname, node.lineno)
