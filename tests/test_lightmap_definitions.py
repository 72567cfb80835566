"""The lightmap post-process definitions against their own past: lightmap_finish, lightmap_finish_sh, lightmap_finish_var (samples as a
number and as a plane) and lightmap_select over every battery the mutants and the kernels are held against, each returned array's SHA-256
compared with tests/golden/lightmap_definitions.json, which was recorded from the helpers of the commit the file names.  A change to the
shared building blocks that moves one bit of one form shows here, whichever form's own tests it slips past.  No GPU."""
import hashlib
import json
import os

import numpy as np
import pytest

from cs397raytracingsp22_amd import lightmap_finish, lightmap_finish_sh, lightmap_finish_var, lightmap_select

import adaptive_batteries as ab
import finish_batteries as fb
import variance_batteries as vb
from test_lightmap_sh_host import BATTERIES as SH_BATTERIES

GOLDEN = os.path.join(fb.ROOT, "tests", "golden", "lightmap_definitions.json")


def digest(a):
    """SHA-256 of the array's dtype, shape and bytes (a plain int counts as an int64 scalar array)"""
    a = np.ascontiguousarray(a)
    h = hashlib.sha256(f"{a.dtype.str} {a.shape} ".encode())
    h.update(a.tobytes())
    return h.hexdigest()


def _finish(b):
    return lightmap_finish(b[1], b[2], b[3], **b[4])


def _finish_sh(b):
    return lightmap_finish_sh(b[1], b[2], b[3], **b[4])


def _finish_var(b):
    return lightmap_finish_var(b[1], b[2], b[3], b[4], b[5], **b[6])


def _finish_var_counts(b):
    return lightmap_finish_var(b[1], b[2], np.full(b[1].shape[:2], b[3], np.uint32), b[4], b[5], **b[6])


def _select(b):
    index, count, err = lightmap_select(b[1], b[2], b[3], b[5], b[6], b[7])
    return index, np.int64(count), err


FORMS = {
    "lightmap_finish": (_finish, lambda: fb.all_batteries(3, 2)),
    "lightmap_finish_sh": (_finish_sh, lambda: SH_BATTERIES),
    "lightmap_finish_var": (_finish_var, lambda: vb.all_batteries(3, 2)),
    "lightmap_finish_var with a counts plane": (_finish_var_counts, lambda: vb.all_batteries(3, 2)),
    "lightmap_select": (_select, lambda: ab.all_batteries() + ab.extreme_batteries()),
}


def compute(form):
    fn, batteries = FORMS[form]
    out = {}
    for b in batteries():
        assert b[0] not in out, b[0]
        out[b[0]] = [digest(a) for a in fn(b)]
    return out


@pytest.mark.parametrize("form", list(FORMS))
def test_definitions_keep_their_recorded_bits(form):
    with open(GOLDEN) as fh:
        want = json.load(fh)["forms"][form]
    got = compute(form)
    assert sorted(got) == sorted(want)
    changed = [name for name in got if got[name] != want[name]]
    assert not changed, changed
