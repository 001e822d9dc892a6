"""The joint between the conditioner (sgm.modules.GeneralConditioner) and the sampling job (cd360.job.Sampler)."""
from __future__ import annotations

import torch


def sampler_rows(c, uc, branches: int, dtype=torch.bfloat16):
    """(c, uc) as GeneralConditioner.get_unconditional_conditioning returns them for bs target prompts (force_ref_zero_embeddings=True, as
    sample.py:155-161 calls it: target rows only) -> (ctx [branches * bs, 77, D], y [branches * bs, Dy]) in the row order job.Sampler
    documents: [uc | uc | c] for 3 branches, [uc | c] for 2.  The order is not restated here: the rows are built by the guider's own
    prepare_inputs, the guider job.Sampler would choose for that branch count."""
    from . import sampler as S
    if branches == 3:
        guider = S.ScheduledCFGImgTextRef(1.0, 1.0)
    elif branches == 2:
        guider = S.VanillaCFGImgRef(1.0)
    else:
        raise ValueError(f"branches must be 2 or 3 (job.Sampler's guiders), got {branches!r}")
    assert guider.branches == branches
    for k in ("crossattn", "vector"):
        if k not in c or k not in uc or c[k].shape != uc[k].shape:
            raise ValueError(f"c and uc must both hold {k!r} of one shape")
    ctx, y = c["crossattn"], c["vector"]
    bs = ctx.shape[0]
    if y.shape[0] != bs:
        raise ValueError(f"crossattn has {bs} rows, vector {y.shape[0]}")
    rows = guider.prepare_inputs(ctx.new_zeros(bs, 1), ctx.new_zeros(bs), {"crossattn": ctx, "vector": y},
                                 {"crossattn": uc["crossattn"], "vector": uc["vector"]})[2]
    return rows["crossattn"].to(dtype).contiguous(), rows["vector"].to(dtype).contiguous()
