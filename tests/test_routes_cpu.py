"""Which kernel does a gpv_gemm / gpv_conv2d call take?  Answered without a GPU: tools/route_host_check.cpp compiles the routing header
(gpv-1_amd/csrc/gemm_route.h) with g++ alone and prints the Route of every case of tests/route_cases.py; the lines must equal
tests/golden/routes/expected.txt (the launches of a kernel trace of tools/route_sweep.py: profiles/r17_routes.txt).  A change of the
selection policy shows here as the cases it moved; regenerate the file with
  python tests/route_cases.py | <the compiled program> > tests/golden/routes/expected.txt
after a kernel trace has confirmed the new launches."""
import os
import re
import shutil
import subprocess

import pytest

from tests import route_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'gpv-1_amd', 'csrc')
EXPECTED = os.path.join(ROOT, 'tests', 'golden', 'routes', 'expected.txt')


@pytest.fixture(scope='module')
def routed(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.fail('g++ is needed to compile tools/route_host_check.cpp')
    exe = str(tmp_path_factory.mktemp('routes') / 'route_host_check')
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-o', exe, os.path.join(ROOT, 'tools', 'route_host_check.cpp')], check=True)
    text = ''.join(route_cases.case_line(c) + '\n' for c in route_cases.CASES)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(l.split(': ', 1) for l in out)


def test_every_case_takes_its_pinned_route(routed):
    expected = dict(l.rstrip('\n').split(': ', 1) for l in open(EXPECTED))
    assert sorted(expected) == sorted(c['name'] for c in route_cases.CASES) == sorted(routed)
    moved = ['%s\n  pinned %s\n  now    %s' % (n, expected[n], routed[n]) for n in expected if routed[n] != expected[n]]
    assert not moved, '%d cases changed their route:\n%s' % (len(moved), '\n'.join(moved))


def test_the_cases_reach_every_family_and_both_sides_of_a_refusal(routed):
    """the table is only worth something if it exercises the whole dispatcher: every family takes some case, some call is refused, the
    stride-2 pointwise backward-data is a route of two parts, and every row of the step's GEMM shapes is there"""
    fams = {r.split(' + ')[0].split()[0] for r in routed.values()}
    assert fams >= {'gemv', 'c1s', 'c3s', 'conv_split', 'pipe', 'skinny', 'glds', 'halo', 'glds_wgrad', 'glds_tt', 'skinny_tt', 'tile', 'refused'}
    assert any(' + s2_fill' in r for r in routed.values())
    import json
    steps = json.load(open(os.path.join(ROOT, 'tools', 'gemm_shapes_step.json')))
    assert sum(c['name'].startswith('step') for c in route_cases.CASES) == len(steps)


def test_the_routing_header_is_host_only():
    """gemm_route.h: no HIP call, no stream, no device type; it includes <stdint.h>, the public header and host_defs.h (tune_env, al16,
    drop_thresh: plain C++ shared with the kernels' common.h) and nothing else"""
    src = open(os.path.join(CSRC, 'gemm_route.h')).read()
    code = re.sub(r'//[^\n]*', '', src)
    for word in ('hipLaunchKernelGGL', 'hipFuncSetAttribute', 'hipStream_t', '__global__', '__device__', 'hip_runtime'):
        assert word not in code, word
    assert re.findall(r'#include\s+(\S+)', code) == ['<stdint.h>', '"../../include/gpv_hip.h"', '"host_defs.h"']
    assert re.findall(r'#include\s+(\S+)', open(os.path.join(CSRC, 'host_defs.h')).read()) == ['<stdint.h>', '<stdlib.h>']


def test_families_are_ordered_once_and_launches_decide_nothing():
    """the order of the families is route_try's alone, and no .hip file tests a shape on the way to a launch: what used to be
    <family>_try_launch is gone, and the one definition of the knobs is gemm.hip's"""
    hips = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith('.hip')}
    assert not any('_try_launch' in s for s in hips.values())
    assert not any(re.search(r'\bextern\s+(int|long)\s+g_\w+_(mode|launches)', s) for s in hips.values())
    assert [f for f, s in hips.items() if re.search(r'^namespace gpvk \{ Knobs g_knobs; \}', s, re.M)] == ['gemm.hip']
    assert not any(re.search(r'\b\w+_select\(', s) for s in hips.values())      # selection is called from route_try only
