#!/usr/bin/env python3
"""Record a digest of every packed weight stream of the fused family in tests/golden/pack_streams.json.

``python tests/golden/make_pack_streams.py COMMIT`` with the library of that commit built: the cases and the digest are
tests/test_pack_layout.py's (PACK_SHAPES, pack_stream_digest), so the file and the test that reads it cannot disagree
about what is hashed; the architectures are the fused family of tests/test_gpu_exact_integer.py, written into the file.  Run once, before a change that must not move a byte of a stream; COMMIT is written into
the file as the commit whose library produced it.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_gpu_exact_integer as X  # noqa: E402
import test_pack_layout as L  # noqa: E402

if __name__ == "__main__":
    archs = {n: X.ARCHS[n] for n in sorted(X.FUSED) + sorted(X.INFER_EXTRA)}
    streams = {"%s-%d" % (n, s): L.pack_stream_digest(a, s) for n, a in archs.items() for s in L.PACK_SHAPES if s != 20 or a["use_viewdirs"]}
    with open(L.PACK_STREAMS_JSON, "w") as f:
        json.dump({"produced_by_commit": sys.argv[1], "architectures": archs, "weights": "synth.make_state_dict(3, 3.0, **arch)", "streams": streams},
                  f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d digests" % len(streams))
