"""Kernel by kernel: is the gfx950 machine code of every kernel symbol the parent's rollout.o
has byte-identical in this build's rollout.o?

  python profiles/rollout_proposals/symbol_text.py PARENT_rollout.o NEW_rollout.o

Each object carries its device code as a clang offload bundle in .hip_fatbin; the gfx950 entry is
unbundled, and for every FUNC symbol of its .text (one per kernel) the symbol's bytes
[value, value + size) are hashed (SHA-256). Prints one line per parent symbol that differs or is
missing, the symbols only this build has, and the summary. A compile, not a run."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get('ROCM_PATH', '/opt/rocm')
LLVM = os.path.join(ROCM, 'lib', 'llvm', 'bin')


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp, tag):
    fat, co = os.path.join(tmp, tag + '.fatbin'), os.path.join(tmp, tag + '.co')
    run(os.path.join(LLVM, 'llvm-objcopy'), '-O', 'binary', '--only-section=.hip_fatbin', obj, fat)
    run(os.path.join(LLVM, 'clang-offload-bundler'), '--unbundle', '--type=o', '--input=' + fat,
        '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--output=' + co)
    return co


def kernels(co):
    """{symbol: (size, sha256 of its bytes)} of the FUNC symbols in .text."""
    readelf = os.path.join(LLVM, 'llvm-readelf')
    text = None
    for line in run(readelf, '-S', '--wide', co).splitlines():
        m = re.match(r'\s*\[\s*(\d+)\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)', line)
        if m:
            text = (int(m.group(1)), int(m.group(2), 16), int(m.group(3), 16), int(m.group(4), 16))
    assert text, 'no .text'
    ndx, addr, off, size = text
    blob = open(co, 'rb').read()
    out = {}
    for line in run(readelf, '-s', '--wide', co).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == 'FUNC' and f[6] == str(ndx):
            v, n = int(f[1], 16), int(f[2])
            assert addr <= v and v + n <= addr + size, f[7]
            out[f[7]] = (n, hashlib.sha256(blob[off + v - addr:off + v - addr + n]).hexdigest())
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        a, b = kernels(code_object(sys.argv[1], tmp, 'parent')), kernels(code_object(sys.argv[2], tmp, 'new'))
    names = run('c++filt', *a, *b).splitlines() if a or b else []
    pretty = dict(zip(list(a) + list(b), names))
    same = 0
    for s, (n, h) in a.items():
        if s not in b:
            print(f'MISSING in this build: {pretty[s]}')
        elif b[s] != (n, h):
            print(f'DIFFERS ({n} vs {b[s][0]} bytes): {pretty[s]}')
        else:
            same += 1
    for s in b:
        if s not in a:
            print(f'new, {b[s][0]} bytes: {pretty[s]}')
    print(f'{same} of the parent\'s {len(a)} kernel symbols have byte-identical code in this build; '
          f'{len(b) - len(set(a) & set(b))} symbols are new')


if __name__ == '__main__':
    main()
