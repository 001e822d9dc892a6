"""The invalidation rule of cached derived weights, on CPU tensors: cd360.derived.derived itself, the process-wide table behind
ops.bias_f32 / ops.weight_t, and two sites that pack without the library (util._fp32_affine, images._conv1x1_pack).

Before the rule had one home, two of these cases served stale values: `p.data = ...` (nn.Module.to) for ops.bias_f32, which looked at
object identity and version only, and `norm.bias = nn.Parameter(...)` for util._fp32_affine, which keyed a bias by its version alone."""
import pytest
import torch
import torch.nn as nn

import derived_cases as DC


def _linear():
    torch.manual_seed(0)
    lin = nn.Linear(4, 4).to(torch.bfloat16).requires_grad_(False)
    with torch.no_grad():
        lin.bias.copy_(torch.arange(1.0, 5.0))  # nn.Linear's own init is fine for the weight; a bias that is surely non-zero
    return lin


class _Site:
    """derived() on a frozen Linear with a counting make()."""

    def __init__(self):
        self.lin, self.calls, self.extra = _linear(), 0, ()

    def make(self):
        self.calls += 1
        return self.lin.weight.detach().float().clone(), self.lin.bias.detach().float().clone()

    def __call__(self):
        from cd360.derived import derived
        return derived(self.lin, "_slot", (self.lin.weight, self.lin.bias), self.make, self.extra)


def _fresh(site):
    return site.lin.weight.detach().float(), site.lin.bias.detach().float()


def test_repeat_call_serves_the_same_object_without_make():
    site = _Site()
    first = site()
    assert site.calls == 1 and site() is first and site() is first and site.calls == 1
    assert "_slot" in site.lin.__dict__  # the entry sits in the owner's __dict__, not behind nn.Module.__setattr__


@pytest.mark.parametrize("attr", ["weight", "bias"])
@pytest.mark.parametrize("mutate", DC.MUTATIONS, ids=lambda f: f.__name__)
def test_each_mutation_is_followed_by_exactly_one_rebuild(mutate, attr):
    site = _Site()
    first = site()
    mutate(site.lin, attr)
    second = site()
    assert second is not first and site.calls == 2
    assert DC.same(second, _fresh(site))
    assert site() is second and site.calls == 2


def test_changed_extra_rebuilds_once():
    site = _Site()
    first = site()
    site.extra = (True,)
    second = site()
    assert second is not first and site.calls == 2 and DC.same(second, _fresh(site))
    assert site() is second and site.calls == 2
    site.extra = (False,)
    assert site() is not second and site.calls == 3


def test_none_source_is_accepted_and_turning_it_into_a_tensor_rebuilds():
    from cd360.derived import derived
    lin = nn.Linear(4, 4, bias=False).requires_grad_(False)
    calls = []

    def make():
        calls.append(1)
        return lin.weight.detach().clone(), None if lin.bias is None else lin.bias.detach().clone()

    first = derived(lin, "_slot", (lin.weight, lin.bias), make)
    assert first[1] is None and derived(lin, "_slot", (lin.weight, lin.bias), make) is first and len(calls) == 1
    lin.bias = nn.Parameter(torch.ones(4), requires_grad=False)
    second = derived(lin, "_slot", (lin.weight, lin.bias), make)
    assert second is not first and len(calls) == 2 and torch.equal(second[1], torch.ones(4))
    assert derived(lin, "_slot", (lin.weight, lin.bias), make) is second and len(calls) == 2


def test_an_edit_through_data_is_not_seen():
    """The documented limit (cd360/derived.py): `.data` is a tensor with a version counter of its own, so `p.data.copy_()` leaves
    object, version, address, dtype and device as they were.  Changing this is a decision, not an accident."""
    from cd360 import ops
    site = _Site()
    first = site()
    b32 = ops.bias_f32(site.lin.bias)
    site.lin.bias.data.copy_(site.lin.bias.data * 0.5)
    assert site() is first and site.calls == 1 and not DC.same(first, _fresh(site))
    assert ops.bias_f32(site.lin.bias) is b32 and not torch.equal(b32, site.lin.bias.detach().float())


# ------------------------------------------------------------------------------------------------ ops.bias_f32 / ops.weight_t
def _ops_sites():
    from cd360 import ops
    return {"bias_f32": (ops.bias_f32, "bias", lambda p: p.detach().float()), "weight_t": (ops.weight_t, "weight", lambda p: p.detach().t().contiguous())}


@pytest.mark.parametrize("name", ["bias_f32", "weight_t"])
def test_ops_table_serves_a_repeat_call(name):
    fn, attr, fresh = _ops_sites()[name]
    lin = _linear()
    first = fn(getattr(lin, attr))
    assert fn(getattr(lin, attr)) is first and torch.equal(first, fresh(getattr(lin, attr)))


@pytest.mark.parametrize("name", ["bias_f32", "weight_t"])
@pytest.mark.parametrize("mutate", DC.MUTATIONS, ids=lambda f: f.__name__)
def test_ops_table_rebuilds_once_after_each_mutation(mutate, name):
    fn, attr, fresh = _ops_sites()[name]
    lin = _linear()
    first = fn(getattr(lin, attr))
    mutate(lin, attr)
    second = fn(getattr(lin, attr))
    assert second is not first
    assert second.dtype == fresh(getattr(lin, attr)).dtype and torch.equal(second, fresh(getattr(lin, attr)))
    assert fn(getattr(lin, attr)) is second


# ------------------------------------------------------------------------------------------------ two sites that need no library
@pytest.mark.parametrize("attr", ["weight", "bias"])
@pytest.mark.parametrize("mutate", DC.MUTATIONS, ids=lambda f: f.__name__)
def test_fp32_affine_follows_its_group_norm(mutate, attr):
    from sgm.modules.diffusionmodules.util import _fp32_affine
    torch.manual_seed(1)
    norm = nn.GroupNorm(2, 4).requires_grad_(False)
    with torch.no_grad():
        norm.weight.copy_(torch.rand(4) + 0.5)
        norm.bias.copy_(torch.rand(4) + 0.5)
    first = _fp32_affine(norm)
    assert DC.served(first, _fp32_affine(norm))
    mutate(norm, attr)
    second = _fp32_affine(norm)
    assert DC.rebuilt(first, second) and DC.same(second, (norm.weight.detach().float(), norm.bias.detach().float()))
    assert DC.served(second, _fp32_affine(norm))


@pytest.mark.parametrize("attr", ["weight", "bias"])
@pytest.mark.parametrize("mutate", DC.MUTATIONS, ids=lambda f: f.__name__)
def test_conv1x1_pack_follows_its_convolution(mutate, attr):
    from cd360 import images
    torch.manual_seed(2)
    conv = nn.Conv2d(4, 4, 1).requires_grad_(False)
    first = images._conv1x1_pack(conv, 4, 4)
    assert DC.served(first, images._conv1x1_pack(conv, 4, 4))
    mutate(conv, attr)
    second = images._conv1x1_pack(conv, 4, 4)
    assert DC.rebuilt(first, second) and DC.same(second, (conv.weight.detach().float().reshape(4, 4), conv.bias.detach().float()))
    assert DC.served(second, images._conv1x1_pack(conv, 4, 4))
