"""`oics` -- host-side mirror of the reference crate's public modules (packages/lib/src/lib.rs:1-12)
over libomrdeskew.so.  Module names follow the crate: calculate, fft, hough, omr, projection, transfer, types; jpeg and png are this project's own.
"""
from . import calculate, fft, hough, jpeg, omr, png, projection, synth, transfer, types  # noqa: F401
from ._lib import LIB_PATH, OmrError, lib  # noqa: F401
