"""What can happen to a parameter behind a cached derived weight (cd360/derived.py), shared by test_derived_cpu.py and
test_derived_gpu.py.  Every mutation takes (module, attribute name) and leaves a parameter of the same shape, dtype and requires_grad whose
values a stale copy would no longer match (the bare version bump aside: there only the rebuild is observable)."""
import torch
import torch.nn as nn


def copy_(mod, attr):
    p = getattr(mod, attr)
    with torch.no_grad():
        p.copy_(p * 0.5 + 0.25)


def load_state_dict(mod, attr):
    sd = {k: v.clone() for k, v in mod.state_dict().items()}
    sd[attr] = sd[attr] * 0.5 + 0.25
    mod.load_state_dict(sd)


def increment_version(mod, attr):
    torch.autograd.graph.increment_version(getattr(mod, attr))


def data_swap(mod, attr):
    """What nn.Module.to(device | dtype) does: the same Parameter object at the same version on another storage."""
    p = getattr(mod, attr)
    obj, version = p, p._version
    p.data = p.data.clone() * 0.5
    assert getattr(mod, attr) is obj and p._version == version


def replace(mod, attr):
    """`mod.bias = nn.Parameter(...)`: another object whose version counter equals the old one's."""
    old = getattr(mod, attr)
    new = nn.Parameter(old.detach().clone() * 0.5 + 0.25, requires_grad=old.requires_grad)
    while new._version < old._version:
        torch.autograd.graph.increment_version(new)
    assert new._version == old._version and new is not old
    setattr(mod, attr, new)


MUTATIONS = (copy_, load_state_dict, increment_version, data_swap, replace)


def tensors(pack):
    """Every tensor of a pack (tuples, lists, dicts, objects with attributes such as FusedNerfWeights), in a fixed order."""
    if isinstance(pack, torch.Tensor):
        return [pack]
    if pack is None or isinstance(pack, (int, float, bool, str)):
        return []
    if isinstance(pack, dict):
        return [t for k in sorted(pack) for t in tensors(pack[k])]
    if isinstance(pack, (tuple, list)):
        return [t for v in pack for t in tensors(v)]
    return tensors(vars(pack))


def same(a, b) -> bool:
    ta, tb = tensors(a), tensors(b)
    return len(ta) == len(tb) and len(ta) > 0 and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(ta, tb))


def served(a, b) -> bool:
    """b is the pack a, served again: the same tensor objects throughout."""
    ta, tb = tensors(a), tensors(b)
    return len(ta) == len(tb) and all(x is y for x, y in zip(ta, tb))


def rebuilt(a, b) -> bool:
    """b shares no tensor object with the pack a."""
    return not {id(t) for t in tensors(a)} & {id(t) for t in tensors(b)}
