#!/usr/bin/env python3
"""Make the HDF5 fixtures of tests/test_dataset.py: the reference's own data files (written by h5py: superblock v0,
v1 object headers, one symbol-table group, contiguous datasets) cut down to their leading samples so that each fits
the repository's file-size limit.

    python tests/golden/make_h5_golden.py /path/to/Multigrid-FEANet

The files are not rewritten through a library: every byte outside the dropped samples is kept, and only the numbers
that must change are patched in place — each dataset's leading dimension (dataspace message, and the layout
message's size), and every file address behind a dropped range (superblock end-of-file and root entry, symbol-table
message, B-tree children, symbol-node entries, local-heap data segment, header continuations, dataset layout),
shifted down by the bytes dropped in front of it.  So feanet_amd.h5lite is still tested on h5py's own encoding.
Prints the data offset of every dataset in the new files (test_dataset.py reads the raw blocks there)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "multigrid-feanet_amd"))
from feanet_amd.h5lite import _UNDEF, File  # noqa: E402

# fixture name -> (file under the reference's Data/, samples kept per dataset; None = all of them)
FILES = {
    "isopoisson_33x33_first10.h5": ("IsoPoisson/poisson2d_33x33.h5", 10),
    "testpoisson_33x33.h5": ("TestPoisson/poisson2d_33x33.h5", None),
    "rhs_17x17_first100_40.h5": ("RHS/poisson2d_rhs_17x17.h5", {"train": 100, "test": 40}),
}


def messages(h, ohdr):
    """(type, data position, size) of every message of a v1 object header, continuation messages included."""
    r, b = h._r, h._mm
    p = ohdr
    assert b[p] == 1, "v1 object header expected"
    nmsg = r.u(p + 2, 2)
    blocks = [(p + 16, r.u(p + 8, 4))]
    seen = 0
    while blocks and seen < nmsg:
        q, size = blocks.pop(0)
        end = q + size
        while q + 8 <= end and seen < nmsg:
            mtype, msize = r.u(q, 2), r.u(q + 2, 2)
            seen += 1
            if mtype == 0x10:
                blocks.append((r.off(q + 8), r.ln(q + 8 + r.so)))
            yield mtype, q + 8, msize
            q += 8 + msize


def shrink(src, dst, keep):
    h = File(src)
    b, r = h._mm, h._r
    so, sl = r.so, r.sl
    assert h._base == 0 and h._find_superblock() == 0
    addr_pos, cuts, patches, datasets = [], [], [], {}

    def entry(e):  # symbol-table entry: name offset, header address, cache type, reserved, scratch pad
        addr_pos.append(e + so)
        if r.u(e + 2 * so, 4) == 1:  # cached B-tree and heap addresses of a group
            addr_pos.extend([e + 2 * so + 8, e + 2 * so + 8 + so])
        return r.off(e + so)

    def btree(p, heap):
        assert b[p:p + 4] == b"TREE"
        level, used = b[p + 5], r.u(p + 6, 2)
        addr_pos.extend([p + 8, p + 8 + so])  # siblings
        q = p + 8 + 2 * so + sl
        for _ in range(used):
            addr_pos.append(q)
            child = r.off(q)
            if level > 0:
                btree(child, heap)
            else:
                assert b[child:child + 4] == b"SNOD"
                e = child + 8
                for _ in range(r.u(child + 6, 2)):
                    datasets[h._heap_name(heap, r.off(e))] = entry(e)
                    e += 2 * so + 24
            q += so + sl

    p = 24 + (4 if b[8] == 1 else 0)
    eof_pos = p + 2 * so
    assert r.off(eof_pos) == len(b)
    addr_pos.append(eof_pos)
    root = entry(p + 4 * so)
    for mtype, q, _ in messages(h, root):
        if mtype == 0x10:
            addr_pos.append(q)
        elif mtype == 0x11:
            addr_pos.extend([q, q + so])
            heap = r.off(q + so)
            assert b[heap:heap + 4] == b"HEAP"
            addr_pos.append(heap + 8 + 2 * sl)
            btree(r.off(q), heap)
    for name, ohdr in datasets.items():
        arr = h[name]
        n = arr.shape[0] if keep is None else keep[name] if isinstance(keep, dict) else keep
        assert 0 < n <= arr.shape[0]
        row = arr[0].nbytes
        for mtype, q, _ in messages(h, ohdr):
            if mtype == 0x10:
                addr_pos.append(q)
            elif mtype == 0x01:
                ver, nd, flags = b[q], b[q + 1], b[q + 2]
                d0 = q + (8 if ver == 1 else 4)
                assert r.ln(d0) == arr.shape[0]
                patches.append((d0, sl, n))
                if flags & 1 and r.ln(d0 + nd * sl) == arr.shape[0]:  # a fixed maximum size follows the dimensions
                    patches.append((d0 + nd * sl, sl, n))
            elif mtype == 0x08:
                ver = b[q]
                if ver == 3:
                    assert b[q + 1] == 1, "contiguous layout expected"
                    apos = q + 2
                    assert r.ln(apos + so) == arr.nbytes
                    patches.append((apos + so, sl, n * row))
                else:
                    assert b[q + 2] == 1, "contiguous layout expected"
                    apos = q + 8
                    assert r.u(apos + so, 4) == arr.shape[0]
                    patches.append((apos + so, 4, n))
                addr_pos.append(apos)
                a = r.off(apos)
                if n < arr.shape[0]:
                    cuts.append((a + n * row, a + arr.nbytes))
    cuts.sort()

    def moved(a):
        assert not any(s < a < e for s, e in cuts), "an address points into dropped samples"
        return a - sum(e - s for s, e in cuts if e <= a)

    out = bytearray(b[:])
    for pos in addr_pos:
        a = r.off(pos)
        if a != _UNDEF:
            out[pos:pos + so] = moved(a).to_bytes(so, "little")
    for pos, nb, val in patches:
        out[pos:pos + nb] = int(val).to_bytes(nb, "little")
    for s, e in reversed(cuts):
        del out[s:e]
    with open(dst, "wb") as fh:
        fh.write(out)
    # read back: every dataset is the leading samples of the original, bit for bit
    with File(dst) as g:
        assert sorted(g.keys()) == sorted(h.keys())
        print(os.path.basename(dst), len(out), "bytes")
        for name, ohdr in sorted(g._root.items()):
            new = np.array(g[name])
            np.testing.assert_array_equal(new, np.array(h[name])[:new.shape[0]])
            off = next(g._r.off(q + (2 if g._mm[q] == 3 else 8)) for mtype, q, _ in messages(g, ohdr) if mtype == 0x08)
            assert bytes(out[off:off + new.nbytes]) == new.tobytes()
            print(f"  {name}: shape {new.shape} {new.dtype}, data at offset {off}")
    h.close()


if __name__ == "__main__":
    ref = os.path.join(sys.argv[1], "Data")
    for fixture, (path, keep) in FILES.items():
        shrink(os.path.join(ref, path), os.path.join(HERE, fixture), keep)
