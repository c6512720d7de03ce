"""Resource usage of the GA && SH instantiations of rollout_persist_kernel beside their SH
siblings, and every other kernel of csrc/rollout.hip against the parent, from two compiles with
-Rpass-analysis=kernel-resource-usage (a compile, not a run):

  hipcc <the flags of build_lib.FLAGS> -Rpass-analysis=kernel-resource-usage \\
        -I include -c csrc/rollout.hip -o /tmp/x.o 2> remarks.txt          # in each tree
  python profiles/rollout_proposals/resource_table.py parent_remarks.txt new_remarks.txt

Prints a markdown table: one row per new instantiation, the sibling's figures behind it."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'imagine_shield'))
from resource_table import KEYS, others, parse, persist  # noqa: E402


def main():
    parent, new = parse(sys.argv[1]), parse(sys.argv[2])
    pp, nn = persist(parent), persist(new)
    fresh = sorted(a for a in nn if a not in pp)
    assert all(a.endswith('true, true') for a in fresh) and len(fresh) == 12, fresh
    print('| RB, NW, LW, PM, PG, GA, SH | ' + ' | '.join(KEYS) + ' | the SH sibling (GA = false): the same columns |')
    print('|' + '---|' * (len(KEYS) + 2))
    for args in fresh:
        sib = nn[args[:-len('true, true')] + 'false, true']
        print(f'| {args} | ' + ' | '.join(str(nn[args].get(k)) for k in KEYS) + ' | ' +
              ' '.join(str(sib.get(k)) for k in KEYS) + ' |')
    po, no = others(parent), others(new)
    print(f'\nthe {len(pp)} instantiations of the parent report the parent\'s figures: '
          f'{all(pp[a] == nn[a] for a in pp)}; the {len(po)} other kernels of rollout.hip too: {po == no}')


if __name__ == '__main__':
    main()
