"""Fixture for tests/test_host_logic.py::test_reference_parameter_files_load_unchanged: the
settings of the parameters files that the reference's own runtime and validation tests use
(Geonomics 1.4.9, tests/runtime/ and tests/validation/), stored as data so that the test does
not need the reference.  Each file's `params` dict is kept as JSON with tags for what JSON
lacks: {"__dict__": [[key, value], ...]} (keeps int keys and key order), {"__tuple__": [...]},
{"__ndarray__": nested list, "dtype": ...}.

    python tests/golden/make_ref_params_fixture.py <reference checkout>  ->  ref_param_files.json
"""
import json
import os
import sys

import numpy as np

FILES = ['tests/runtime/runtime_params.py',
         'tests/runtime/runtime_params_selection.py',
         'tests/validation/bottleneck/bottleneck_params.py',
         'tests/validation/wf/wf_params.py']


def encode(o):
    if isinstance(o, dict):
        return {'__dict__': [[k, encode(v)] for k, v in o.items()]}
    if isinstance(o, tuple):
        return {'__tuple__': [encode(v) for v in o]}
    if isinstance(o, list):
        return [encode(v) for v in o]
    if isinstance(o, np.ndarray):
        return {'__ndarray__': o.tolist(), 'dtype': str(o.dtype)}
    assert o is None or isinstance(o, (bool, int, float, str)), type(o)
    return o


if __name__ == '__main__':
    ref = sys.argv[1]
    out = {}
    for rel in FILES:
        ns = {}
        exec(open(os.path.join(ref, rel)).read(), ns)
        out[rel] = encode(ns['params'])
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ref_param_files.json')
    with open(dst, 'w') as f:
        json.dump(out, f, separators=(',', ':'))
    print('wrote', dst)
