"""Committed fixtures under tests/golden/.  A fixture is <tag>.npz; one whose arrays would make a file larger than the 1 MiB limit of a
committed file continues in <tag>.part2.npz, <tag>.part3.npz, ... (whole arrays per file, written by save_fixture)."""
import io
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILE_LIMIT = 1 << 20


def _part_path(path, k):
    return path if k == 1 else f"{path[:-4]}.part{k}.npz"


def load(tag):
    """{name: array} of every file of fixture `tag`."""
    path = os.path.join(GOLD, tag + ".npz")
    out, k = {}, 1
    while os.path.exists(_part_path(path, k)):
        with np.load(_part_path(path, k)) as z:
            out.update({n: z[n] for n in z.files})
        k += 1
    if not out:
        raise FileNotFoundError(path)
    return out


def _compressed_size(arr):
    buf = io.BytesIO()
    np.savez_compressed(buf, a=arr)
    return buf.tell()


def save_fixture(path, fx, limit=FILE_LIMIT - (32 << 10)):
    """np.savez_compressed of `fx` at `path` (<tag>.npz), spilling whole arrays into <tag>.part2.npz, ... when one file would pass
    `limit` bytes.  Returns the list of files written."""
    parts, size = [{}], [0]
    for n, a in fx.items():
        s = _compressed_size(np.asarray(a))
        if parts[-1] and size[-1] + s > limit:
            parts.append({})
            size.append(0)
        parts[-1][n] = a
        size[-1] += s
    k = 2
    while os.path.exists(_part_path(path, k)):            # continuation files of an earlier, larger version
        os.remove(_part_path(path, k))
        k += 1
    files = []
    for k, part in enumerate(parts, 1):
        np.savez_compressed(_part_path(path, k), **part)
        files.append(_part_path(path, k))
    return files
