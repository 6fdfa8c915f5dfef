"""One memo for the fp64 references (a helper: no tests in here).  The references are the slow
part of the suite and several test modules ask for the same ones; `memo` computes each once per
process and hands the same read-only array to every caller."""
import inspect

import numpy as np


def array(dtype):
    """normaliser of an array argument: contiguous, of the stated dtype"""
    return lambda a: np.ascontiguousarray(a, dtype)


def memo(**norm):
    """@memo(x=array(np.float32), scale=float, lock=bool): memoise a reference on its full
    arguments.  A named argument goes through its normaliser first (None stays None), the
    others as they are; the function is called with the normalised values.  An ndarray enters the
    key as (dtype, shape, bytes), the bytes themselves, so two inputs never share an entry.
    The result is an ndarray, returned read-only, the same object for the same call."""
    def deco(fn):
        sig = inspect.signature(fn)
        store = {}

        def cached(*args, **kw):
            bound = sig.bind(*args, **kw)
            bound.apply_defaults()
            vals = [norm[k](v) if k in norm and v is not None else v for k, v in bound.arguments.items()]
            key = tuple((v.dtype.str, v.shape, v.tobytes()) if isinstance(v, np.ndarray) else v for v in vals)
            if key not in store:
                out = fn(*vals)
                out.setflags(write=False)
                store[key] = out
            return store[key]
        cached.__doc__ = fn.__doc__
        return cached
    return deco
