"""Resource usage of every rollout_persist_kernel instantiation, parent against this build,
from two compiles of csrc/rollout.hip with -Rpass-analysis=kernel-resource-usage (a
compile, not a run). profiles/imagine_shield/resource_table.py with one difference: the
parent has the seventh template argument too, so every instantiation has a counterpart.

  hipcc <the flags of build_lib.FLAGS> -Rpass-analysis=kernel-resource-usage \\
        -I include -c csrc/rollout.hip -o /tmp/x.o 2> remarks.txt          # in each tree
  python profiles/imagine_linear/resource_table.py parent_remarks.txt new_remarks.txt

Prints a markdown table of the new build's instantiations; a row is marked `same` when
every figure the compiler reports equals the parent's, else the parent's figures follow."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'imagine_shield'))
from resource_table import KEYS, others, parse, persist  # noqa: E402


def main():
    parent, new = parse(sys.argv[1]), parse(sys.argv[2])
    pp, nn = persist(parent), persist(new)
    assert set(pp) == set(nn), 'the instantiations changed'
    print('| RB, NW, LW, PM, PG, GA, SH | ' + ' | '.join(KEYS) + ' | against the parent |')
    print('|' + '---|' * (len(KEYS) + 2))
    for args, fig in sorted(nn.items()):
        note = 'same' if pp[args] == fig else 'parent: ' + ' '.join(str(pp[args].get(k)) for k in KEYS)
        print(f'| {args} | ' + ' | '.join(str(fig.get(k)) for k in KEYS) + f' | {note} |')
    po, no = others(parent), others(new)
    sh_false = [a for a in nn if a.endswith('false')]
    print(f'\n{len(sh_false)} SH = false instantiations identical: {all(pp[a] == nn[a] for a in sh_false)}; '
          f'the {len(po)} other kernels of rollout.hip identical: {po == no}')


if __name__ == '__main__':
    main()
