#!/usr/bin/env python3
"""Is the device code of two builds the same?  tools/code_object_diff.py BUILD_A BUILD_B [--arch gfx950]

For every rsl_*.o of the two build directories (radar-slam_amd/build of two trees): the gfx950 code object is taken out
of the object's .hip_fatbin section and unbundled, and the hashes of its .text and .rodata sections and of its notes
(llvm-readelf --notes: kernel names, argument layouts, register and LDS use) are printed side by side.  The code object
as a whole carries a per-build id, so it differs between two builds of one source; these three do not.  Exit status 1
when any file differs or is in one directory only."""
import argparse
import glob
import hashlib
import os
import subprocess
import sys
import tempfile

LLVM = os.environ.get('ROCM_LLVM', '/opt/rocm/llvm/bin')


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True).stdout


def hashes(obj, arch, tmp):
    fat, co, sec = (os.path.join(tmp, n) for n in ('fatbin', 'code_object', 'section'))
    run('llvm-objcopy', '-O', 'binary', '--only-section=.hip_fatbin', obj, fat)
    if os.path.getsize(fat) == 0:  # host code only (rsl_api.o)
        return ['no device code'] * 3
    run('clang-offload-bundler', '--unbundle', '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--' + arch,
        '--input=' + fat, '--output=' + co)
    out = []
    for name in ('.text', '.rodata'):
        run('llvm-objcopy', '-O', 'binary', '--only-section=' + name, co, sec)
        with open(sec, 'rb') as f:
            out.append(hashlib.sha256(f.read()).hexdigest()[:16])
    out.append(hashlib.sha256(run('llvm-readelf', '--notes', co)).hexdigest()[:16])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('build_a')
    ap.add_argument('build_b')
    ap.add_argument('--arch', default='gfx950')
    a = ap.parse_args()
    names = sorted({os.path.basename(p) for d in (a.build_a, a.build_b) for p in glob.glob(os.path.join(d, 'rsl_*.o'))})
    differ = 0
    print(f'{"object":26s} {"text":>35s} {"rodata":>35s} {"notes":>35s}')
    with tempfile.TemporaryDirectory() as tmp:
        for n in names:
            pa, pb = os.path.join(a.build_a, n), os.path.join(a.build_b, n)
            if not (os.path.exists(pa) and os.path.exists(pb)):
                print(f'{n:26s} only in {a.build_a if os.path.exists(pa) else a.build_b}')
                differ += 1
                continue
            ha, hb = hashes(pa, a.arch, tmp), hashes(pb, a.arch, tmp)
            cols = ' '.join(f'{x:>35s}' for x in (u if u == v else u + ' / ' + v for u, v in zip(ha, hb)))
            print(f'{n:26s} {cols}{"" if ha == hb else "  DIFFERS"}')
            differ += ha != hb
    print(f'{len(names)} objects, {differ} differ')
    return 1 if differ else 0


if __name__ == '__main__':
    sys.exit(main())
