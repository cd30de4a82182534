# Final-build verification, round 6: differential soak, the whole GPU suite, the bench (contract line), smoke
OUT=${OUT:?set OUT to the directory the results go to}
python tools/fuzz_paillier.py 300 6201 2>&1 | tail -1 > "$OUT/r06_fuzz_final.txt"
python tools/fuzz_gpu.py 120 6202 2>&1 | tail -1 >> "$OUT/r06_fuzz_final.txt"
timeout 2400 python -m pytest tests -m gpu -q -x 2>&1 | tail -6 > "$OUT/r06_gpu_suite_final3.txt"
timeout 900 python bench.py --full > "$OUT/r06_bench_final3.line.json" 2> "$OUT/r06_bench_final3.err"
cp bench_detail.json "$OUT/r06_bench_final3.json"
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$OUT/r06_smoke_final3.txt" 2>&1
