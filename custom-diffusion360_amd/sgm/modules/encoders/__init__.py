"""The conditioner's embedders (modules.py)."""
