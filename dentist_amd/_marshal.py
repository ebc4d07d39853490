"""What every command of the binding does with its arguments and results: pointers of arrays, the mask pair with its
sentinels, the offsets of concatenated sequences, views and copies of library memory, and the owner of a handle."""
import ctypes

import numpy as np

from ._abi import lib


def addr(a):
    """The data pointer of an array; None for an empty or absent one."""
    return a.ctypes.data if a is not None and len(a) else None


def mask_pair(mask, n=None, short="a mask's ptr needs n + 1 entries", name="mask"):
    """(ptr, iv) -> ptr as int64 and the intervals as flat int32 with the two sentinel zeros behind them.  n: the
    sequences the mask is over -- ptr must have n + 1 entries (`short` is the message otherwise) and must not point
    behind the intervals; None: as given, the library checks."""
    mp = np.ascontiguousarray(mask[0], dtype=np.int64)
    mi = np.ascontiguousarray(np.concatenate([np.asarray(mask[1], dtype=np.int32).reshape(-1), [0, 0]]), dtype=np.int32)
    if n is not None:
        if len(mp) != n + 1:
            raise ValueError(short)
        if len(mp) and 2 * int(mp.max()) > len(mi) - 2:
            raise ValueError(f"the {name}'s ptr lies behind the end of its intervals")
    return mp, mi


def optional_mask(mask):
    """mask_pair of a mask that may be None, as the calls with a repeat mask take it: (the arrays, to be kept alive until
    the call returns; the address of ptr; the address of the intervals) -- three times None without a mask."""
    if mask is None:
        return None, None, None
    mp, mi = mask_pair(mask)
    return (mp, mi), mp.ctypes.data, mi.ctypes.data


def seq_pairs(ref, ref_off, qry, qry_off, same_count=True):
    """Two sets of concatenated sequences as (uint8, int64 offsets) each, the offsets checked: n + 1 entries (the same
    n on both sides unless same_count is False) that stay inside their sequences."""
    r, q = np.ascontiguousarray(ref, dtype=np.uint8), np.ascontiguousarray(qry, dtype=np.uint8)
    roff, qoff = np.ascontiguousarray(ref_off, dtype=np.int64), np.ascontiguousarray(qry_off, dtype=np.int64)
    if len(roff) < 1 or len(qoff) < 1 or (same_count and len(roff) != len(qoff)):
        raise ValueError("ref_off and qry_off need n + 1 entries each")
    if (len(roff) > 1 and int(roff.max()) > len(r)) or (len(qoff) > 1 and int(qoff.max()) > len(q)):
        raise ValueError("an offset lies behind the end of the sequences")
    return r, roff, q, qoff


def _address(p):
    return p if isinstance(p, int) else ctypes.cast(p, ctypes.c_void_p).value


def view(p, count, dtype, owner):
    """`count` items of `dtype` at the library's address p as a numpy view; `owner` stays alive as long as the view."""
    if not count:
        return np.zeros(0, dtype=dtype)
    buf = (ctypes.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(_address(p))
    buf._owner = owner
    return np.frombuffer(buf, dtype=dtype)


def copy(p, shape, dtype):
    """An array of `shape` and `dtype` copied out of the library's memory at p (sizes beyond 2 GB included)."""
    a = np.zeros(shape, dtype=dtype)
    if a.nbytes:
        ctypes.memmove(a.ctypes.data, p, a.nbytes)
    return a


class Owner:
    """A handle of the library and the function that destroys it.  A subclass names the function in `_destroy` and may
    say in _owned() that the handle is not (or no longer) its own to destroy."""
    _destroy = None

    def __init__(self, h):
        self._h = h

    def _owned(self):
        return True

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and self._owned():
            getattr(lib(), self._destroy)(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
