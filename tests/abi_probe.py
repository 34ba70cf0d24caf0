"""Plumbing of tests/test_abi_cpu.py (and of the library-specific tests that read a header): the comment-stripped header, what it
declares, what a built library exports and imports, the prototypes as class strings, and the gcc offsetof probe.  The header parse
and the nm call are the ones __graft_entry__.build() checks every build with."""
import ctypes
import importlib
import os
import re
import subprocess

import __graft_entry__ as entry
from gpv1_amd import _native

LIBRARIES = _native.LIBRARIES
exported = entry._exported
header_path = _native.header_path


def module(key):
    return importlib.import_module(_native.module_name(key))


def built(key):
    """path of the library the binding module loads, built first if it is not there"""
    if not os.path.exists(module(key)._LIB_PATH):
        entry.build()
    return module(key)._LIB_PATH


def source(key):
    return entry._header_source(header_path(key))


def declared(key):
    return entry._declared(header_path(key), LIBRARIES[key].prefix)


def imports(path):
    """nm -D --undefined-only: what the library takes from others"""
    return subprocess.run(['nm', '-D', '--undefined-only', path], capture_output=True, text=True, check=True).stdout


_C_CLASS = {'int': 'i', 'float': 'f', 'int64_t': 'q', 'long long': 'q', 'uint64_t': 'Q', 'unsigned long long': 'Q'}
_CTYPES_CLASS = {'P': 'P', 'z': 'P', 'i': 'i', 'f': 'f', 'l': 'q', 'q': 'q', 'L': 'Q', 'Q': 'Q'}


def prototypes(key):
    """{entry point: one letter per parameter} from the header: P pointer, i int, f float, q int64_t / long long, Q uint64_t"""
    out = {}
    for name, params in re.findall(r'\bint\s+(' + LIBRARIES[key].prefix + r'\w+)\s*\(([^)]*)\)\s*;', source(key)):
        params = [] if params.strip() == 'void' else params.split(',')
        out[name] = ''.join('P' if '*' in p else _C_CLASS[' '.join(p.replace('const ', ' ').split()[:-1])] for p in params)
    return out


def argtypes_classes(fn):
    """the same string from a ctypes function's argtypes: c_void_p, c_char_p and POINTER(...) all count as pointer"""
    code = lambda t: t._type_ if isinstance(getattr(t, '_type_', None), str) else 'P'
    return ''.join(_CTYPES_CLASS[code(t)] for t in fn.argtypes)


def c_layout(tmp_path, headers, pairs):
    """{C struct name: (sizeof, [offsetof of every field of the ctypes mirror])} of the (name, ctypes class) pairs, from a gcc-compiled probe"""
    prog = ['#include <stdio.h>', '#include <stddef.h>'] + [f'#include "{h}"' for h in headers] + ['int main(void) {']
    for cname, cls in pairs:
        prog.append(f'  printf("{cname} %zu", sizeof({cname}));')
        for f, _ in cls._fields_:
            prog.append(f'  printf(" %zu", offsetof({cname}, {f}));')
        prog.append('  printf("\\n");')
    prog += ['  return 0;', '}']
    c = tmp_path / 'probe.c'
    c.write_text('\n'.join(prog))
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-std=c99', '-o', str(exe), str(c)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    return {l.split()[0]: (int(l.split()[1]), [int(v) for v in l.split()[2:]]) for l in lines}


def ctypes_layout(cls):
    return ctypes.sizeof(cls), [getattr(cls, f).offset for f, _ in cls._fields_]
