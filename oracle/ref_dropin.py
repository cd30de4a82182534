"""The drop-in check of include/ipcl, as a build step: the reference's OWN client sources (test/, benchmark/, example/)
are compiled unchanged, where they lie in the reference tree (never copied into this repository), against include/ipcl
and the two stand-in headers under tests/cpp/shims (googletest / google-benchmark, syntax only).

build() runs this and writes the outcome to oracle/_ref/dropin.json (git-ignored; it travels with the built tree);
tests/test_dropin_compile.py reads only that record.  The record names the headers it was made against (a digest of
include/ and tests/cpp/shims), so a stale one is caught.  Where the reference tree is absent an existing record is kept."""
import glob
import hashlib
import json
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("IPCL_REFERENCE_DIR", "/root/reference")      # where the reference checkout lives
RECORD = os.path.join(ROOT, "oracle", "_ref", "dropin.json")
DIRS = ("test", "benchmark", "example")


def header_digest():
    """sha256 over the files the check compiles against: include/ and tests/cpp/shims/"""
    h = hashlib.sha256()
    for d in ("include", os.path.join("tests", "cpp", "shims")):
        for dp, dns, fns in os.walk(os.path.join(ROOT, d)):
            dns.sort()
            for f in sorted(fns):
                p = os.path.join(dp, f)
                h.update(os.path.relpath(p, ROOT).encode() + b"\0")
                with open(p, "rb") as fh:
                    h.update(fh.read())
    return h.hexdigest()


def client_sources(ref=REF):
    """the reference's client sources, relative to its tree"""
    return sorted(os.path.relpath(s, ref) for d in DIRS for s in glob.glob(os.path.join(ref, d, "*.cpp")))


def _compile(rel):
    cmd = ["g++", "-std=c++17", "-fopenmp", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "tests", "cpp", "shims"), os.path.join(REF, rel)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    return {"returncode": r.returncode, "stderr": r.stderr[-3000:]}


def build(force=False):
    """compile every client source (syntax and types) into the record; a no-op while the record matches the headers"""
    found = client_sources()
    if not found or shutil.which("g++") is None:
        return None
    digest = header_digest()
    if not force and os.path.exists(RECORD):
        with open(RECORD) as f:
            old = json.load(f)
        if old.get("headers_sha256") == digest and old.get("found") == found:
            return RECORD
    with ThreadPoolExecutor(max_workers=min(len(found), len(os.sched_getaffinity(0)), 8)) as ex:
        results = dict(zip(found, ex.map(_compile, found)))
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    with open(RECORD, "w") as f:
        json.dump({"found": found, "headers_sha256": digest, "results": results}, f, indent=1)
    return RECORD
