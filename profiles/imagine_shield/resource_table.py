"""Resource usage of every rollout_persist_kernel instantiation, parent against this build,
from two compiles of csrc/rollout.hip with -Rpass-analysis=kernel-resource-usage (a
compile, not a run):

  hipcc <the flags of build_lib.FLAGS> -Rpass-analysis=kernel-resource-usage \\
        -I include -c csrc/rollout.hip -o /tmp/x.o 2> remarks.txt          # in each tree
  python profiles/imagine_shield/resource_table.py parent_remarks.txt new_remarks.txt

Prints a markdown table of the new build's instantiations; an SH = false row is marked
`same` when every figure the compiler reports equals the parent's instantiation with the
same first six template arguments."""
import collections
import re
import subprocess
import sys

KEYS = ['VGPRs', 'AGPRs', 'TotalSGPRs', 'SGPRs Spill', 'VGPRs Spill', 'ScratchSize [bytes/lane]',
        'Occupancy [waves/SIMD]', 'LDS Size [bytes/block]']


def parse(path):
    out, cur = collections.OrderedDict(), None
    for line in open(path):
        m = re.search(r'remark:\s+Function Name: (\S+)', line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r'remark:\s+([A-Za-z \[\]/]+?): (\S+) \[-Rpass', line)
        if m and cur:
            out[cur][m.group(1).strip()] = m.group(2)
    return out


def demangle(names):
    return subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')


def persist(table):
    """{template arguments: figures} of the rollout_persist_kernel instantiations."""
    names = [n for n in table if 'rollout_persist_kernel' in n]
    return {re.search(r'rollout_persist_kernel<(.*?)>', d).group(1): table[n] for n, d in zip(names, demangle(names))}


def others(table):
    """{demangled name: figures} of the file's other kernels."""
    names = [n for n in table if 'rollout_persist_kernel' not in n]
    return dict(zip(demangle(names), (table[n] for n in names)))


def main():
    parent, new = parse(sys.argv[1]), parse(sys.argv[2])
    pp = {k + ', false': v for k, v in persist(parent).items()}       # the parent has no seventh argument
    print('| RB, NW, LW, PM, PG, GA, SH | ' + ' | '.join(KEYS) + ' | against the parent |')
    print('|' + '---|' * (len(KEYS) + 2))
    for args, fig in sorted(persist(new).items()):
        if args in pp:
            note = 'same' if all(pp[args].get(k) == fig.get(k) for k in pp[args]) else \
                'DIFFERS: ' + ' '.join(str(pp[args].get(k)) for k in KEYS)
        else:
            note = 'new'
        print(f'| {args} | ' + ' | '.join(str(fig.get(k)) for k in KEYS) + f' | {note} |')
    po, no = others(parent), others(new)
    print(f'\n{len(pp)} parent instantiations; the {len(po)} other kernels of rollout.hip identical: '
          f'{all(po[n] == no.get(n) for n in po)}')


if __name__ == '__main__':
    main()
