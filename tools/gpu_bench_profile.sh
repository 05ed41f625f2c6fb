cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
# the full bench line, its rocprofv3 kernel trace and the two PMC passes, into $OUT (default profile_out/)
OUT=${OUT:-profile_out} && mkdir -p "$OUT" && \
timeout -k 10 300 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err" && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats -T -d "$OUT/prof_kt" -o kt --output-format csv -- python bench.py --full --steps 50 --warmup 5 --no-cpu-baseline > "$OUT/prof_kt.log" 2>&1 && \
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE -T -d "$OUT/prof_fetch" -o fetch --output-format csv -- python bench.py --full --steps 5 --warmup 1 --knn-steps 1 --no-cpu-baseline --no-exchange > "$OUT/prof_fetch.log" 2>&1 && \
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE -T -d "$OUT/prof_write" -o write --output-format csv -- python bench.py --full --steps 5 --warmup 1 --knn-steps 1 --no-cpu-baseline --no-exchange > "$OUT/prof_write.log" 2>&1
