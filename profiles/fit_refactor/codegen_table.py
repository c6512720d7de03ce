"""Per-kernel code-generation comparison of two builds, from hipcc --save-temps output.

    python profiles/fit_refactor/codegen_table.py PARENT_DIR NEW_DIR file [file ...]

DIR/<file>-hip-amdgcn-amd-amdhsa-gfx950.s is what `hipcc <build_lib.FLAGS> --save-temps -c
csrc/<file>.hip` leaves in its working directory. Per kernel: the instruction text with
comments dropped and local labels renumbered in order of appearance (identical / differs),
the instruction count, and from the code object metadata VGPR / SGPR / VGPR spills + SGPR
spills / scratch bytes / static LDS. Prints a markdown table per file."""
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    meta = {}
    for blk in re.split(r'\n  - \.agpr_count:', text)[1:]:
        f = {k: v for k, v in re.findall(r'\.(\w+):\s+(\S+)', blk.split('\namdhsa.target')[0])}
        meta[f['name']] = f
    out = {}
    for name in meta:
        body = re.search(r'^%s:[^\n]*\n(.*?)^\.Lfunc_end' % re.escape(name), text, re.S | re.M).group(1)
        lines, labels = [], {}
        for ln in body.split('\n'):
            ln = ln.split(';')[0].strip()
            if ln:
                lines.append(ln)
        for ln in lines:
            for lab in re.findall(r'\.LBB\d+_\d+', ln):
                labels.setdefault(lab, f'.L{len(labels)}')
        lines = [re.sub(r'\.LBB\d+_\d+', lambda mm: labels[mm.group(0)], ln) for ln in lines]
        insts = [ln for ln in lines if not ln.endswith(':') and not ln.startswith('.')]
        f = meta[name]
        res = '%s / %s / %s+%s / %s / %s' % (f['vgpr_count'], f['sgpr_count'], f['vgpr_spill_count'],
                                             f['sgpr_spill_count'], f['private_segment_fixed_size'],
                                             f['group_segment_fixed_size'])
        out[name] = ('\n'.join(lines), len(insts), res)
    return out


def demangle(names):
    r = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True)
    return dict(zip(names, (x.split('(')[0] for x in r.stdout.split('\n'))))


def main():
    pdir, ndir = sys.argv[1:3]
    for f in sys.argv[3:]:
        suffix = f'/{f}-hip-amdgcn-amd-amdhsa-gfx950.s'
        a, b = kernels(pdir + suffix), kernels(ndir + suffix)
        dm = demangle(sorted(set(a) | set(b)))
        print(f'\n### {f}.hip\n\n| kernel | text | instructions parent / new | parent | new |\n|---|---|---|---|---|')
        for k in sorted(dm, key=dm.get):
            if k in a and k in b:
                same = 'identical' if a[k][0] == b[k][0] else 'differs'
                print(f'| `{dm[k]}` | {same} | {a[k][1]} / {b[k][1]} | {a[k][2]} | {b[k][2]} |')
            elif k in a:
                print(f'| `{dm[k]}` | removed | {a[k][1]} / - | {a[k][2]} | - |')
            else:
                print(f'| `{dm[k]}` | new | - / {b[k][1]} | - | {b[k][2]} |')


if __name__ == '__main__':
    main()
