#!/usr/bin/env python3
"""Digest of the device code: what a refactor of the host text must leave alone.

Compiles every source of the engine device-only for gfx950 in both precisions (the flags of professad_amd._build), unbundles
the code object and prints, per translation unit and precision, the sorted kernel symbols with, for each,

    <unit> <precision> <size of the code in bytes> <hash of the kernel descriptor> <hash of the disassembly> <symbol>

The disassembly is hashed without addresses (branch targets are relative), the descriptor without its offset to the code, so
two builds whose kernels only sit in another order give the same digest.  `diff` of two digests names every kernel that
changed, appeared or went away.  Needs no GPU.

    python tools/device_code_digest.py > after.txt                 # every unit, both precisions
    python tools/device_code_digest.py --summarise after.txt       # one line per unit and precision (what profiles/ keeps)
    python tools/device_code_digest.py --units lines.hip --precisions f32 -- -DOFDFT_NO_MIXED_F32
"""
import argparse
import concurrent.futures
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from professad_amd import _build  # noqa: E402

LLVM = os.environ.get('ROCM_LLVM', '/opt/rocm/llvm/bin')
PRECISIONS = {'f64': [], 'f32': ['-DOFDFT_REAL_F32', '-cl-single-precision-constant']}      # as _build.build
BUNDLE_MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'


def code_object(src, flags, tmp):
    """device-only compile of one source -> path of its gfx950 ELF"""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    out = os.path.join(tmp, 'dev.out')
    subprocess.run([hipcc] + _build._flags(flags) + ['--offload-device-only', '-c', os.path.join(_build.CSRC, src), '-o', out],
                   check=True)
    with open(out, 'rb') as fh:
        bundled = fh.read(len(BUNDLE_MAGIC)) == BUNDLE_MAGIC
    if not bundled:
        return out
    elf = os.path.join(tmp, 'dev.co')
    subprocess.run([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o', '--targets=' + TARGET, '--input=' + out,
                    '--output=' + elf, '--unbundle'], check=True)
    return elf


def elf_symbols(path):
    """{name: (value, size, type)} of an ELF64 little-endian object, and a reader of the bytes at a virtual address"""
    with open(path, 'rb') as fh:
        data = fh.read()
    if data[:6] != b'\x7fELF\x02\x01':
        raise SystemExit('%s: not a little-endian ELF64 object' % path)
    shoff, = struct.unpack_from('<Q', data, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', data, 0x3A)
    secs = [struct.unpack_from('<IIQQQQIIQQ', data, shoff + i * shentsize) for i in range(shnum)]
    syms = {}
    for sec in secs:
        if sec[1] != 2:          # SHT_SYMTAB
            continue
        stroff = secs[sec[6]][4]
        for off in range(sec[4], sec[4] + sec[5], 24):
            name, info, _other, shndx, value, size = struct.unpack_from('<IBBHQQ', data, off)
            end = data.index(b'\0', stroff + name)
            syms[data[stroff + name:end].decode()] = (value, size, info & 15, shndx)

    def read(shndx, addr, n):
        sec = secs[shndx]
        return data[sec[4] + addr - sec[3]:sec[4] + addr - sec[3] + n]
    return syms, read


_HEAD = re.compile(r'^(?:[0-9a-f]+ )?<(.+)>:$')


def disassembly(path):
    """{symbol: text of its instructions, addresses and comments stripped}"""
    txt = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', '--no-leading-addr', path], check=True,
                         capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in txt.splitlines():
        m = _HEAD.match(line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip() not in ('', '...'):          # ('...': zero padding up to the next function)
            cur.append(line.split('//')[0].strip())
    return {k: '\n'.join(v) for k, v in out.items()}


def digest(src, prec, extra):
    with tempfile.TemporaryDirectory() as tmp:
        elf = code_object(src, PRECISIONS[prec] + extra, tmp)
        syms, read = elf_symbols(elf)
        dis = disassembly(elf)
    lines = []
    for name in sorted(syms):
        if name + '.kd' not in syms or syms[name][2] != 2:      # a kernel: a function with a descriptor
            continue
        kd_addr, kd_size, _t, kd_sec = syms[name + '.kd']
        kd = bytearray(read(kd_sec, kd_addr, kd_size))
        kd[16:24] = bytes(8)          # kernel_code_entry_byte_offset: where the code sits relative to the descriptor
        lines.append('%s %s %d %s %s %s' % (src, prec, syms[name][1], hashlib.sha256(bytes(kd)).hexdigest()[:16],
                                            hashlib.sha256(dis.get(name, '').encode()).hexdigest()[:16], name))
    return lines


def summary(lines):
    """one line per unit and precision of a full digest: <unit> <precision> <kernels> <code bytes> <hash of its lines, sorted>"""
    groups = {}
    for ln in lines:
        f = ln.split()
        groups.setdefault((f[0], f[1]), []).append(ln.strip())
    return ['%s %s %d %d %s' % (u, p, len(g), sum(int(ln.split()[2]) for ln in g),
                                hashlib.sha256('\n'.join(sorted(g)).encode()).hexdigest()[:32])
            for (u, p), g in groups.items()]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--units', nargs='*', default=_build.SOURCES)
    ap.add_argument('--precisions', nargs='*', default=list(PRECISIONS), choices=list(PRECISIONS))
    ap.add_argument('--jobs', type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument('--summary', action='store_true', help='one line per unit and precision instead of one per kernel')
    ap.add_argument('--summarise', metavar='FILE', help='compile nothing: print the summary of a full digest saved earlier')
    ap.add_argument('extra', nargs='*', help='further compiler flags, after --')
    a = ap.parse_args()
    if a.summarise:
        with open(a.summarise) as fh:
            print('\n'.join(summary(fh.read().splitlines())))
        return
    jobs = [(u, p) for u in a.units for p in a.precisions]
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
        for lines in ex.map(lambda j: digest(j[0], j[1], a.extra), jobs):
            for ln in (summary(lines) if a.summary else lines):
                print(ln)
            sys.stdout.flush()


if __name__ == '__main__':
    main()
