#!/usr/bin/env python3
"""Re-export the reference's shipped ES policy (backup_models/es_swing.dat) as a small .npz fixture, WITHOUT unpickling it.

The .dat file is a torch zip archive whose data.pkl pickles a 1-D float32 numpy array. The pickle is only disassembled
(pickletools.genops yields its opcodes and never executes one): the array's bytes are the BINUNICODE payload of 4 P latin-1
characters that follows its (P,) shape and the 'f4' dtype. Output: tests/golden/es_swing_policy.npz with the P = 766 floats,
the archive member's name and the sha256 of the float32 bytes.

    python tools/export_es_policy.py REFERENCE_CHECKOUT      (or TB_REFERENCE=...)"""
import hashlib
import os
import pickletools
import sys
import zipfile

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "es_swing_policy.npz")
P = 766  # GatedCNN(6, 6)


def weights_from_pickle(data, n=P):
    """the n little-endian float32 values of the one BINUNICODE string of 4 n characters that follows the shape (n,) and dtype f4"""
    saw_shape = saw_f4 = False
    found = []
    for op, arg, _ in pickletools.genops(data):
        if op.name in ("BININT", "BININT1", "BININT2") and arg == n:
            saw_shape = True
        elif isinstance(arg, str) and arg == "f4":
            saw_f4 = True
        elif op.name in ("BINUNICODE", "SHORT_BINUNICODE", "BINUNICODE8") and isinstance(arg, str) and len(arg) == 4 * n:
            found.append(arg)
    if not (saw_shape and saw_f4) or len(found) != 1:
        raise SystemExit("data.pkl does not hold exactly one (%d,) f4 array payload" % n)
    return np.frombuffer(found[0].encode("latin-1"), dtype="<f4").copy()


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TB_REFERENCE")
    if not ref:
        raise SystemExit(__doc__)
    z = zipfile.ZipFile(os.path.join(ref, "backup_models", "es_swing.dat"))
    member = [m for m in z.namelist() if m.endswith("/data.pkl")]
    if len(member) != 1:
        raise SystemExit("expected one data.pkl in the archive, found %r" % member)
    w = weights_from_pickle(z.read(member[0]))
    sha = hashlib.sha256(w.astype("<f4").tobytes()).hexdigest()
    np.savez_compressed(OUT, weights=w, member=np.array(member[0]), sha256=np.array(sha))
    print("wrote", os.path.normpath(OUT), w.shape, member[0], sha)


if __name__ == "__main__":
    sys.exit(main())
