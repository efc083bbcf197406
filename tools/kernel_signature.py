#!/usr/bin/env python
"""Signatures of the device code, the twin of plan_signature.py - no GPU needed.  Every .hip file named on the command line
(default: build.SOURCES; a bare name is looked up in yoloret_amd/csrc) is compiled with build.FLAGS plus -S --cuda-device-only,
and one line is printed per kernel: the mangled name and the SHA-256 of that kernel's assembly text, from its label to the end of
its .amdhsa_kernel descriptor (code, register and LDS budget).  The __hip_cuid_* symbol lines, which differ from one compile to
the next, are dropped.  A change that claims to leave the device code alone prints the same text before and after:
    python tools/kernel_signature.py mbxr_h.hip mbr.hip > after.txt
--csrc DIR reads the sources from another tree (a checkout of the parent commit) with the same flags."""
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yoloret_amd import build   # noqa: E402


def assembly(path):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    return subprocess.run([hipcc] + build.FLAGS + ['-S', '--cuda-device-only', path, '-o', '-'], check=True,
                          stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode()


def kernels(asm):
    """[(mangled name, sha256 of the kernel's text)] in the file's order."""
    lines = [l for l in asm.split('\n') if '__hip_cuid_' not in l]
    names = [m.group(1) for m in (re.match(r'\s*\.amdhsa_kernel\s+(\S+)', l) for l in lines) if m]
    start = {m.group(1): i for i, m in enumerate(re.match(r'([^\s.][^\s:]*):', l) for l in lines) if m}
    rows = []
    for name in names:
        end = next(i for i in range(start[name], len(lines)) if lines[i].strip() == '.end_amdhsa_kernel')
        rows.append((name, hashlib.sha256('\n'.join(lines[start[name]:end + 1]).encode()).hexdigest()))
    return rows


def main():
    args = sys.argv[1:]
    csrc = build.CSRC
    if '--csrc' in args:
        i = args.index('--csrc')
        csrc = args[i + 1]
        del args[i:i + 2]
    paths = [a if os.path.sep in a else os.path.join(csrc, a) for a in (args or build.SOURCES)]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        for path, asm in zip(paths, pool.map(assembly, paths)):
            rows = kernels(asm)
            print('%s: %d kernels' % (os.path.basename(path), len(rows)))
            for name, digest in rows:
                print('  %s %s' % (name, digest))


if __name__ == '__main__':
    main()
