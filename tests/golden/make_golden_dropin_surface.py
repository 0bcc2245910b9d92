"""Writes tests/golden/dropin_surface.json: the interface the reference's train.py / test.py / collect_data.py expect of dropin/,
read off their syntax trees -- every `from <module> import <names>` of each script, and the dotted attribute reads of train.py on
the objects the shims hand out.  Names only; nothing of the scripts themselves.

    python tests/golden/make_golden_dropin_surface.py <reference checkout>
"""
import ast
import json
import os
import sys

SCRIPTS = ("train.py", "test.py", "collect_data.py")
TRAIN_ROOTS = {"envs", "actor_critic", "rollouts", "agent", "algo_args", "config", "env_config"}   # train.py's local names of shim objects


def import_froms(tree):
    return [[n.module, [a.name for a in n.names]] for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and n.module]


def attr_chains(tree, roots):
    """dotted attribute reads `root.a.b` for the given root variable names"""
    out = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute):
            parts, cur = [node.attr], node.value
            while isinstance(cur, ast.Attribute):
                parts.append(cur.attr)
                cur = cur.value
            if isinstance(cur, ast.Name) and cur.id in roots:
                out.add((cur.id,) + tuple(reversed(parts)))
    return [list(c) for c in sorted(out)]


def main():
    ref = sys.argv[1]
    trees = {s: ast.parse(open(os.path.join(ref, s)).read()) for s in SCRIPTS}
    out = {"import_from": {s: import_froms(t) for s, t in trees.items()},
           "train_py_attr_chains": attr_chains(trees["train.py"], TRAIN_ROOTS)}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin_surface.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path, {s: len(v) for s, v in out["import_from"].items()}, len(out["train_py_attr_chains"]))


if __name__ == "__main__":
    main()
