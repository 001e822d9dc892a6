"""`sgm.modules.GeneralConditioner` (the YAML target of configs/train_co3d_concept.yaml:56-57) resolves lazily: importing this package
imports no encoder module and loads no shared library, so it works in a tree that has not been built."""


def __getattr__(name):
    if name == "GeneralConditioner":
        from .encoders.modules import GeneralConditioner
        return GeneralConditioner
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
