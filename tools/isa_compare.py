#!/usr/bin/env python3
"""Per-kernel comparison of two device assemblies of csrc/sr_device.hip (hipcc -S --cuda-device-only):
   tools/isa_compare.py OLD.s NEW.s
For every function: sha256 of its instructions (label to .Lfunc_end; the __hip_cuid_<hash> word, which follows the
source text, replaced by a fixed one) and the .amdhsa_ / resource figures of its kernel descriptor that matter here
(VGPRs, SGPRs, spills, scratch, LDS, code bytes).  Prints one row per function: equal or the figures side by side."""
import hashlib
import re
import subprocess
import sys

KEYS = ("NumVgprs", "NumAgprs", "NumSgprs", "ScratchSize", "Occupancy", "codeLenInByte", "LDSByteSize")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def functions(path):
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(path).read())
    out, name, body = {}, None, []
    for ln in text.splitlines():
        m = re.match(r"^(_Z\w+|sr_\w+):\s*(;.*)?$", ln)
        if name is None and m:
            name, body = m.group(1), []
            continue
        if name is not None:
            if ln.startswith(".Lfunc_end"):
                out[name] = {"sha": hashlib.sha256("\n".join(body).encode()).hexdigest()[:16]}
                cur, name = name, None
                out[cur]["_open"] = True
            else:
                body.append(ln)
        for k in KEYS:   # the "; NumVgprs: 256" comment block after each function
            m2 = re.match(r"^;\s*%s\s*[:=]\s*(\d+)" % k, ln)
            if m2:
                last = [n for n, v in out.items() if v.get("_open")]
                if last:
                    out[last[-1]][k] = int(m2.group(1))
    for v in out.values():
        v.pop("_open", None)
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    names = sorted(set(a) | set(b))
    dm = demangle(names)
    differ = 0
    for n in names:
        fa, fb = a.get(n), b.get(n)
        short = re.sub(r"^void ", "", dm[n])[:72]
        if fa == fb:
            print("%-72s equal  %s  vgpr %s scratch %s code %s" % (short, fa["sha"], fa.get("NumVgprs"),
                                                                    fa.get("ScratchSize"), fa.get("codeLenInByte")))
        else:
            differ += 1
            print("%-72s DIFFERS" % short)
            for tag, f in (("old", fa), ("new", fb)):
                print("    %s %s" % (tag, f and " ".join("%s=%s" % kv for kv in sorted(f.items()))))
    print("%d functions, %d differ" % (len(names), differ))


if __name__ == "__main__":
    main()
