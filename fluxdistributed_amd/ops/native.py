"""Loader for the in-tree HIP extension (fluxdistributed_amd/_C*.so).

The extension is compiled for gfx950 only (see csrc/ and setup.py); it is
built in-tree so the .so travels with the repo snapshot to GPU machines.
"""

import os
import threading


_NATIVE = None
_TRIED = False
_LOCK = threading.Lock()


def load_native():
    """Import the compiled extension, caching the result. Returns module or None."""
    global _NATIVE, _TRIED
    if _TRIED:
        return _NATIVE
    # Replica threads (parallel/task_ddp.py) can get here together on the
    # first step. _TRIED is set only once the import has finished, under the
    # lock: a thread arriving while another is still loading the .so (slow
    # when the file is cold) must wait for it, not see "tried, and absent".
    with _LOCK:
        if _TRIED:
            return _NATIVE
        try:
            from fluxdistributed_amd import _C  # noqa: F401  (in-tree .so)

            _NATIVE = _C
        except ImportError:
            _NATIVE = None
        _TRIED = True
    return _NATIVE


def native_available() -> bool:
    return load_native() is not None


def require_native(opname: str):
    """Return the native module; raise loudly if we are on a GPU without it.

    On a GPU box the HIP path must be the one that runs — a silent eager
    fallback would let GPU tests pass without exercising native code.
    """
    mod = load_native()
    if mod is None:
        raise RuntimeError(
            f"fluxdistributed_amd native extension is required for op '{opname}' "
            "on GPU tensors but fluxdistributed_amd._C is not importable. "
            "Build it with: python setup.py build_ext --inplace "
            "(PYTORCH_ROCM_ARCH=gfx950)."
        )
    return mod


def allow_eager_gpu_fallback() -> bool:
    """Escape hatch for debugging only (FLUXDIST_ALLOW_EAGER=1)."""
    return os.environ.get("FLUXDIST_ALLOW_EAGER", "0") == "1"
