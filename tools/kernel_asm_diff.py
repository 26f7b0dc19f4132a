#!/usr/bin/env python3
"""tools/kernel_asm_diff.py OLD.s NEW.s -- which kernels of two `hipcc -S --cuda-device-only` listings have the same instruction stream.

Make the listings with the Makefile's flags, e.g. in fredholm_amd/csrc of each of the two trees:
    hipcc $(FLAGS) -S --cuda-device-only render.hip -o render.s
Every function (kernel or device function) is cut out at its label and compared line by line, comments stripped and the function-local label numbers
(.LBB<function>_<block>, jump tables, .Ltmp, .Lpost_getpc) normalised: a function added in front of another renumbers that one's labels and changes nothing else.
A function whose name only one listing has is matched against the other listing's such functions with its own mangled name replaced inside its body: a kernel
that was renamed (another template argument list, say) and kept its stream prints as RENAMED, not as one GONE and one NEW.
Prints the functions that differ, are renamed, are new or are gone, and the counts; exit status 0 always (it reports, the reader judges)."""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name], name = body, None
                continue
            t = re.sub(r"\.L(BB|JTI|func_begin|func_end|tmp|post_getpc)\d+(_\d+)?", lambda m: ".L" + m.group(1) + (m.group(2) or ""), line.split(";")[0].rstrip())
            if t.strip():
                body.append(t)
    return out


def renamed(a, b):
    """pairs (old, new) of the functions only a / only b has whose bodies are the same once each one's own name is a placeholder; each function pairs once, in name order"""
    def anonymous(fns, k):
        return tuple(line.replace(k, "@SELF") for line in fns[k])
    free = {}
    for k in sorted(set(b) - set(a)):
        free.setdefault(anonymous(b, k), []).append(k)
    pairs = []
    for k in sorted(set(a) - set(b)):
        names = free.get(anonymous(a, k))
        if names:
            pairs.append((k, names.pop(0)))
    return pairs


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    pairs = renamed(a, b)
    paired = {k for pair in pairs for k in pair}
    same = differ = 0
    for k in sorted(set(a) | set(b)):
        if k in paired:
            continue
        if k not in a:
            print("NEW   ", k)
        elif k not in b:
            print("GONE  ", k)
        elif a[k] == b[k]:
            same += 1
        else:
            differ += 1
            print("DIFFER", k, len(a[k]), "->", len(b[k]), "lines")
    for old, new in pairs:
        print("RENAMED", old, "->", new)
    print(f"identical: {same}, different: {differ}")
    print(f"renamed-identical: {len(pairs)}")


if __name__ == "__main__":
    main()
