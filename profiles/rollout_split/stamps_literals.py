"""Stamps build (-DDRPO_STAMPS): where a kernel of this build's rollout.o is not byte-identical to
the parent's, is the difference only the displacement to g_stamps_roll?

  python profiles/rollout_split/stamps_literals.py NEW_stamps_rollout.o PARENT_stamps_rollout.o

A stamped kernel forms the address of g_stamps_roll (.bss of the object's gfx950 code object)
as s_getpc_b64 + s_add_u32 <32-bit literal>. The literal is the distance from the instruction
to .bss, resolved when the code object is linked, so it depends on how much code lies between:
an object with fewer kernels has another distance in the same instruction. For every kernel
symbol both objects have, this prints the number of differing bytes and checks that each lies
in the literal of such a pair and that both literals resolve to g_stamps_roll. A compile, not a
run."""
import os
import struct
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'rollout_proposals'))
import symbol_text as st   # noqa: E402

GETPC, ADD_LIT = 0xBE801C00, 0x8000FF00   # s_getpc_b64 sN; s_add_u32 sN, sN, <literal>


def load(obj, tmp, tag):
    co = st.code_object(obj, tmp, tag)
    readelf = os.path.join(st.LLVM, 'llvm-readelf')
    text, syms = None, {}
    for line in st.run(readelf, '-S', '--wide', co).splitlines():
        f = line.replace('[', ' ').replace(']', ' ').split()
        if len(f) > 4 and f[1] == '.text':
            text = (f[0], int(f[3], 16), int(f[4], 16))
    for line in st.run(readelf, '-s', '--wide', co).splitlines():
        f = line.split()
        if len(f) == 8 and (f[7] == 'g_stamps_roll' or (f[3] == 'FUNC' and f[6] == text[0])):
            syms[f[7]] = (int(f[1], 16), int(f[2]))
    return open(co, 'rb').read(), text, syms


def main():
    with tempfile.TemporaryDirectory() as tmp:
        new, parent = load(sys.argv[1], tmp, 'new'), load(sys.argv[2], tmp, 'parent')
    same = lit = bad = 0
    for s, (va, n) in new[2].items():
        if s == 'g_stamps_roll' or s not in parent[2]:
            continue
        code, addr = [], []
        for blob, (ndx, a0, off), syms in (new, parent):
            v = syms[s][0]
            code.append(blob[off + v - a0:off + v - a0 + n])
            addr.append(v)
        if parent[2][s][1] != n:
            bad += 1
            print(f'DIFFERENT SIZE: {s}')
            continue
        diff = [i for i in range(n) if code[0][i] != code[1][i]]
        if not diff:
            same += 1
            continue
        ok = True
        for w in sorted({i & ~3 for i in diff}):   # the 4-byte literal behind getpc (4) + add (4)
            for k, (blob, text, syms) in enumerate((new, parent)):
                getpc, add, disp = struct.unpack_from('<IIi', code[k], w - 8)
                target = addr[k] + w - 4 + disp    # s_getpc returns the address of the next instruction
                ok &= (getpc & 0xFF80FFFF) == GETPC and (add & 0xFF80FF00) == ADD_LIT
                ok &= target == syms['g_stamps_roll'][0]
        lit += ok
        bad += not ok
        print(f'{len(diff)} bytes differ, {"all in the displacement to g_stamps_roll" if ok else "NOT ONLY THERE"}: '
              f'{st.run("c++filt", s).strip()}')
    print(f'{same} kernel symbols byte-identical, {lit} identical but for the displacement to g_stamps_roll, '
          f'{bad} different otherwise')


if __name__ == '__main__':
    main()
