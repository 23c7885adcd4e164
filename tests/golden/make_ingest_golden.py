#!/usr/bin/env python3
"""Golden fixtures for the native COLLADA ingest (include/rrt.h rrt_collada_load).

TEST INFRASTRUCTURE ONLY (build container; needs /root/reference and oracle/_ref/ref_render,
built by `make -C oracle/ref`).  For every scene asset the reference ships, runs the reference's
own loader through the oracle harness in dump-only mode (`ref_render -Q -r W H`: Collada parser
-> Application::load -> get_static_scene, Camera::configure/place/set_screen_size) and records
the SHA-256 of the flattened scene (.rrts) and camera record (.rrtc) it writes.  Every asset is
also stored (as input data) under tests/golden/dae/ so the ingest tests run without the reference:
as is, xz-compressed when it is over the size limit for a committed file, or -- the near-copies of
another asset -- as line edits of that asset in variants.json (tests/golden_cases.py dae_input
reads all three forms).

Output: tests/golden/ingest.json = {scene: {"src": relative path under dae/, "w": W, "h": H,
"rrts_sha256": ..., "rrtc_sha256": ..., "bytes": n, "committed": bool}}
"""
import difflib
import hashlib
import json
import lzma
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
GOLD = os.path.join(ROOT, "tests", "golden")
DAE = "/root/reference/pathtracer/dae"
BIN = os.path.join(ROOT, "oracle", "_ref", "ref_render")
W, H = 64, 48
FILE_LIMIT = 1 << 20  # bytes: the size limit for a file committed from now on
# near-copies of another asset (a changed light colour, an added microfacet block): stored as edits
VARIANT_OF = {"CBbunny_microfacet_cu": "CBbunny", "bunny_microfacet_cu": "bunny", "bunny_unlit": "bunny",
              "bunny_microfacet_cu_unlit": "bunny", "CBspheres_tex": "CBspheres"}


def variant_ops(base_path, path):
    """[[i, j, lines]]: replacing base lines [i, j) by `lines` (ascending i) turns base into path."""
    a = open(base_path, encoding="utf-8", newline="").read().splitlines(keepends=True)
    b = open(path, encoding="utf-8", newline="").read().splitlines(keepends=True)
    sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
    return [[i1, i2, b[j1:j2]] for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal"]


def store_inputs(srcs):
    """Store every asset {name: path} under tests/golden/dae/ -> {name: stored as a plain copy}."""
    plain, variants = {}, {}
    for name, src in sorted(srcs.items()):
        dst = os.path.join(GOLD, "dae", name + ".dae")
        plain[name] = False
        if name in VARIANT_OF:
            variants[name] = {"base": VARIANT_OF[name], "ops": variant_ops(srcs[VARIANT_OF[name]], src)}
        elif os.path.exists(dst) or os.path.getsize(src) <= FILE_LIMIT:
            shutil.copy(src, dst)  # (assets committed before the limit stay as they are)
            plain[name] = True
        else:
            with open(src, "rb") as f, lzma.open(dst + ".xz", "wb", preset=9 | lzma.PRESET_EXTREME) as g:
                g.write(f.read())
    with open(os.path.join(GOLD, "dae", "variants.json"), "w") as fh:
        json.dump(variants, fh, indent=1, sort_keys=True)
    return plain


def asset_paths():
    out = {}
    for sub in sorted(os.listdir(DAE)):
        for f in sorted(os.listdir(os.path.join(DAE, sub))):
            if f.endswith(".dae"):
                out[f[:-4]] = os.path.join(DAE, sub, f)
    return out


def main():
    out = {}
    tmp = tempfile.mkdtemp()
    srcs = asset_paths()
    plain = store_inputs(srcs)
    for name, src in srcs.items():
        pre = os.path.join(tmp, name)
        subprocess.run([BIN, "-Q", "-r", str(W), str(H), "-O", pre, src], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        size = os.path.getsize(src)
        out[name] = {"src": os.path.relpath(src, DAE), "w": W, "h": H, "bytes": size, "committed": plain[name],
                     "rrts_sha256": hashlib.sha256(open(pre + ".rrts", "rb").read()).hexdigest(),
                     "rrtc_sha256": hashlib.sha256(open(pre + ".rrtc", "rb").read()).hexdigest()}
        print(name, size, "copied" if plain[name] else "stored compressed or as edits")
    with open(os.path.join(GOLD, "ingest.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
