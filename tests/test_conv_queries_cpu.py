"""Truth table of the four conv ``*_has_kernel*`` queries (csrc/lrp_conv.hip), pinned.

The engine picks its entry points by these answers (engine/schedule.py), so a changed answer changes
which kernels a model runs.  The queries do no device work: this runs without a GPU.

``tests/golden/conv_has_kernel.json`` holds, per query, the axes swept and the answers as one string
of 0/1 in row-major order of those axes.  It was recorded from the library with

    python tests/test_conv_queries_cpu.py --record

at the commit before the conv host code got its single lookup per direction; record it again only
when a kernel table or a query's pre-condition changes on purpose.

Axes: the channel widths of the two models' trunks (GTZAN 1-32-32-64-64-128, VGGish 1-64-...-128
with its 100-channel variant, which pads to 128), every pairing of them, W in {8, 16, 24, 32, 256},
every ng 0..4, the forward pool modes 0..3, dense / pool-sparse g, and pool widths 0, 2, 3, 4.
"""
import itertools
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_has_kernel.json")

_CH, _W, _NG = [1, 32, 64, 100, 128], [8, 16, 24, 32, 256], [0, 1, 2, 3, 4]
# query -> (argument names in call order, values per argument)
QUERIES = {
    "drsa_amd_conv_fwd_has_kernel": (("cin", "cout", "W", "ng", "pool", "bf16"), (_CH, _CH, _W, _NG, [0, 1, 2, 3], [0, 1])),
    "drsa_amd_conv_bwd_has_kernel_bf16": (("cin", "cout", "W", "ng", "sparse"), (_CH, _CH, _W, _NG, [0, 1])),
    "drsa_amd_conv_bwd_has_kernel_pw": (("cin", "cout", "W", "ng", "pool_w"), (_CH, _CH, _W, _NG, [0, 2, 3, 4])),
    "drsa_amd_conv_bwd_has_kernel_bf16_pw": (("cin", "cout", "W", "pool_w"), (_CH, _CH, _W, [0, 2, 3, 4])),
}


def _table(name):
    from drsa_audio_amd import _capi
    fn = getattr(_capi.lib(), name)
    return "".join(str(fn(*args)) for args in itertools.product(*QUERIES[name][1]))


@pytest.mark.parametrize("name", sorted(QUERIES))
def test_has_kernel_truth_table(name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    names, axes = QUERIES[name]
    assert want["args"] == list(names) and want["axes"] == [list(a) for a in axes]
    got = _table(name)
    assert set(got) <= {"0", "1"} and len(got) == len(want["answers"])
    bad = [dict(zip(names, args), got=g, want=w)
           for args, g, w in zip(itertools.product(*axes), got, want["answers"]) if g != w]
    assert not bad, bad[:10]
    assert "1" in got and "0" in got


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    sys.path.insert(0, ROOT)
    with open(GOLDEN, "w") as f:
        json.dump({n: {"args": list(QUERIES[n][0]), "axes": [list(a) for a in QUERIES[n][1]], "answers": _table(n)}
                   for n in sorted(QUERIES)}, f, indent=1)
        f.write("\n")
