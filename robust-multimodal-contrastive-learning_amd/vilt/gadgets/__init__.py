"""Mirrors the reference's vilt/gadgets: the epoch metrics (my_metrics.py)."""
