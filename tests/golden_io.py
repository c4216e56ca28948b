"""Loader for the committed golden vectors (tests/golden/*.npz).

An archive that would exceed the size limit for a committed file (1 MiB) is stored as parts
`<stem>.partNN.npz`; every array lives whole in one part and `load_npz` merges them, so the
tests read `<stem>.npz` by name whether it is one file or several."""
import glob
import io
import json
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PART_BYTES = 900 * 1024     # budget of one part (compressed arrays + zip headers stay under 1 MiB)
_cache = {}
_npz = {}


def _parts(path):
    return sorted(glob.glob(path[:-len(".npz")] + ".part[0-9][0-9].npz"))


def load_npz(name):
    """{array name: array} of the golden archive `name` (a file name under tests/golden/ or a path)."""
    path = name if os.path.isabs(name) else os.path.join(GOLDEN, name)
    if path not in _npz:
        files = [path] if os.path.exists(path) else _parts(path)
        if not files:
            raise FileNotFoundError(path)
        arrays = {}
        for f in files:
            z = np.load(f, allow_pickle=False)
            for k in z.files:
                assert k not in arrays, f"{k} in more than one part of {name}"
                arrays[k] = z[k]
        _npz[path] = arrays
    return _npz[path]


def save_parts(path, arrays):
    """np.savez_compressed(path, **arrays), split into `<stem>.partNN.npz` files of at most PART_BYTES
    (by each array's own deflated size) when one file would be larger. Used by the make_golden_* scripts."""
    for f in _parts(path) + [path]:
        if os.path.exists(f):
            os.remove(f)
    sizes = {}
    for k, v in arrays.items():
        buf = io.BytesIO()
        np.save(buf, np.asarray(v), allow_pickle=False)
        sizes[k] = len(zlib.compress(buf.getvalue())) + 2 * len(k) + 128      # + local and central zip headers
        assert sizes[k] <= PART_BYTES, f"{k}: one array over the part budget"
    parts, used = [[]], 0
    for k in arrays:
        if parts[-1] and used + sizes[k] > PART_BYTES:
            parts.append([])
            used = 0
        parts[-1].append(k)
        used += sizes[k]
    if len(parts) == 1:
        np.savez_compressed(path, **arrays)
        return [path]
    out = []
    for i, keys in enumerate(parts):
        out.append(f"{path[:-len('.npz')]}.part{i:02d}.npz")
        np.savez_compressed(out[-1], **{k: arrays[k] for k in keys})
    return out


def load(name):
    if name not in _cache:
        arrays = dict(load_npz(name))
        meta = json.loads(str(arrays.pop("meta")))
        _cache[name] = (arrays, meta)
    return _cache[name]


def case(name, family, i):
    arrays, meta = load(name)
    prefix = f"{family}/{i}/"
    return {k[len(prefix):]: v for k, v in arrays.items() if k.startswith(prefix)}, meta[family][i]


def count(name, family):
    return len(load(name)[1][family])
