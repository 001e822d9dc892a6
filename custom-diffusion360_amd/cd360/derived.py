"""The one invalidation rule of every cached derived weight (packed convolution weights, fp32 affine vectors, LayerNorm-folded Linears,
merged q|k|v, phase kernels, ...): `derived(owner, slot, sources, make)`.  cd360.ops._cached states the same rule for tensors that have
no owner module (its process-wide table), csrc_host/cd360_host.cpp::cached mirrors that one in C++."""
from __future__ import annotations


def derived(owner, slot: str, sources, make, extra=()):
    """make() cached on owner under slot; rebuilt when the sources or extra changed.

    `sources`: a sequence of tensors (None entries allowed) that make() reads; `extra`: anything that is not a tensor and compares with ==
    (a merge flag).  The entry is served while, for every source,
      - it is the same OBJECT as at build time: `mod.bias = nn.Parameter(...)` installs a new tensor whose version counter may well equal the
        old one's.  The entry keeps the source objects, so neither an id nor an address can be recycled while it lives;
      - `_version` is the same: `copy_` under no_grad, `load_state_dict`, an optimizer step and finetune's `bump_versions` write in place;
      - `data_ptr()`, `dtype` and `device` are the same: `nn.Module.to(device | dtype)` assigns `param.data = ...`, which moves the storage
        under an unchanged Parameter object and version;
    and `extra` compares equal.

    The entry lives in `owner.__dict__[slot]`, never behind nn.Module.__setattr__ (slow, and overridden by BasicTransformerBlock and
    SpatialTransformer).  Autograd is the caller's business: a site whose sources are on a tape returns live tensors and does not come here.

    Limit: an edit through `p.data` (`p.data.copy_(...)`) is NOT seen: `.data` is a tensor with a version counter of its own."""
    ent = owner.__dict__.get(slot)
    if ent is not None and ent[1] == extra and len(ent[0]) == len(sources):
        for t, (kept, ptr, version, dtype, device) in zip(sources, ent[0]):
            if t is not kept or (t is not None and (t.data_ptr() != ptr or t._version != version or t.dtype != dtype or t.device != device)):
                break
        else:
            return ent[2]
    stamps = [(t, None, None, None, None) if t is None else (t, t.data_ptr(), t._version, t.dtype, t.device) for t in sources]
    val = make()
    owner.__dict__[slot] = (stamps, extra, val)
    return val
