// tests/host/rollout_targets_check.cpp -- TEST INFRASTRUCTURE.  The host half of csrc/mg_targets.hpp without a GPU and without a GPU compiler: what
// mg_rollout_targets and mg_sum_columns refuse, the overlap check, and -- with a file of cases as argv[1] -- the column walk the kernel runs, here on
// the host over buffers of exactly the sizes the ABI asks for, compared bit for bit with the bits tests/test_rollout_targets_host.py wrote from the
// definition.  Built with -ffp-contract=off -fsanitize=address,undefined and run as a program; prints "OK" and exits 0, or says what failed and exits 1.
//
// The file: int32 cases; per case int32 K, N, has_steps_of, has_skip, has_trunc, has_final, float32 gamma, lam; reward f32[K*N], done u8[K*N],
// value f32[(K+1)*N], the optional arrays that are there (steps_of i32[N], skip u8[K*N], trunc u8[K*N], final f32[K*N]); then what is expected:
// adv f32[K*N], ret f32[K*N], valid u8[K*N], col f64[3*N], sums f64[3].
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../endless-memory-gym_amd/csrc/mg_targets.hpp"

using namespace mg;

static int fail(const char* what) {
    printf("FAILED: %s\n", what);
    return 1;
}

static bool says(const char* got, const char* want) { return got && strstr(got, want); }

// a buffer of exactly `bytes` bytes read from the file (the sanitizer sees a walk that leaves it)
static void* take(FILE* f, size_t bytes) {
    void* p = malloc(bytes ? bytes : 1);
    if (bytes && fread(p, 1, bytes, f) != bytes) {
        printf("FAILED: the cases file is short\n");
        exit(1);
    }
    return p;
}

template <int T>
static void walk(const TargetArrays& A, int K, int N, float gamma, float gl) {
    const bool extra = A.skip || A.trunc || A.final_value;
    for (int i = 0; i < N; ++i) {
        if (extra && A.col) targets_walk_column<T, true, true>(A, K, N, i, gamma, gl);
        else if (extra) targets_walk_column<T, true, false>(A, K, N, i, gamma, gl);
        else if (A.col) targets_walk_column<T, false, true>(A, K, N, i, gamma, gl);
        else targets_walk_column<T, false, false>(A, K, N, i, gamma, gl);
    }
}

static int run_cases(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return fail("the cases file does not open");
    int32_t cases = 0;
    if (fread(&cases, 4, 1, f) != 1 || cases < 1) return fail("the cases file has no cases");
    for (int c = 0; c < cases; ++c) {
        int32_t h[6];
        float g[2];
        if (fread(h, 4, 6, f) != 6 || fread(g, 4, 2, f) != 2) return fail("a case's head");
        const int K = h[0], N = h[1];
        const size_t kn = (size_t)K * N;
        TargetArrays A = {};
        A.reward = (const float*)take(f, kn * 4);
        A.done = (const uint8_t*)take(f, kn);
        A.value = (const float*)take(f, (kn + N) * 4);
        if (h[2]) A.steps_of = (const int32_t*)take(f, (size_t)N * 4);
        if (h[3]) A.skip = (const uint8_t*)take(f, kn);
        if (h[4]) A.trunc = (const uint8_t*)take(f, kn);
        if (h[5]) A.final_value = (const float*)take(f, kn * 4);
        float* want_adv = (float*)take(f, kn * 4);
        float* want_ret = (float*)take(f, kn * 4);
        uint8_t* want_valid = (uint8_t*)take(f, kn);
        double* want_col = (double*)take(f, (size_t)3 * N * 8);
        double* want_sum = (double*)take(f, 3 * 8);
        if (rollout_targets_refusal(A, K, N, g[0], g[1]) == nullptr) return fail("a case without outputs was accepted");
        const float gl = g[0] * g[1];
        // every block length the walk is built for here: 1 (a row at a time), 5 (blocks that do not divide K) and the kernel's own
        for (int pass = 0; pass < 6; ++pass) {
            const bool with_col = pass < 3;
            A.adv = (float*)malloc(kn * 4);
            A.ret = (float*)malloc(kn * 4);
            A.valid = (uint8_t*)malloc(kn);
            A.col = with_col ? (double*)malloc((size_t)3 * N * 8) : nullptr;
            memset(A.adv, 0xA5, kn * 4);
            memset(A.ret, 0xA5, kn * 4);
            memset(A.valid, 0xA5, kn);
            if (const char* no = rollout_targets_refusal(A, K, N, g[0], g[1])) return fail(no);
            if (pass % 3 == 0) walk<1>(A, K, N, g[0], gl);
            else if (pass % 3 == 1) walk<5>(A, K, N, g[0], gl);
            else walk<TARGETS_T>(A, K, N, g[0], gl);
            if (memcmp(A.adv, want_adv, kn * 4) || memcmp(A.ret, want_ret, kn * 4) || memcmp(A.valid, want_valid, kn)) {
                printf("case %d (K %d, N %d), pass %d\n", c, K, N, pass);
                return fail("adv / ret / valid differ from the definition's bits");
            }
            if (with_col) {
                if (memcmp(A.col, want_col, (size_t)3 * N * 8)) return fail("col differs from the definition's bits");
                double sums[3];
                for (int r = 0; r < 3; ++r) sums[r] = sum_columns_row(A.col + (size_t)r * N, N);
                if (memcmp(sums, want_sum, sizeof(sums))) return fail("the sums of the columns differ from the definition's bits");
            }
            free(A.adv);
            free(A.ret);
            free(A.valid);
            free(A.col);
            A.adv = A.ret = nullptr;
            A.valid = nullptr;
            A.col = nullptr;
        }
        free((void*)A.reward);
        free((void*)A.done);
        free((void*)A.value);
        free((void*)A.steps_of);
        free((void*)A.skip);
        free((void*)A.trunc);
        free((void*)A.final_value);
        free(want_adv);
        free(want_ret);
        free(want_valid);
        free(want_col);
        free(want_sum);
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    alignas(16) static char in[1 << 16], out[1 << 16];
    const int K = 6, N = 10;  // K * N floats are 240 bytes, (K + 1) * N floats 280, 3 * N doubles 240
    const float nan = __builtin_nanf("");
    TargetArrays ok = {};
    ok.reward = (const float*)in;
    ok.done = (const uint8_t*)(in + 1024);
    ok.value = (const float*)(in + 2048);
    ok.adv = (float*)out;

    // mg_rollout_targets: what is refused
    if (rollout_targets_refusal(ok, K, N, 0.99f, 0.95f) || rollout_targets_refusal(ok, 1, 1, 0.0f, 1.0f) || rollout_targets_refusal(ok, 1, N, 1.0f, 0.0f))
        return fail("a legal call was refused");
    TargetArrays a = ok;
    a.reward = nullptr;
    if (!says(rollout_targets_refusal(a, K, N, 0.9f, 0.9f), "reward_dev is NULL")) return fail("a NULL reward_dev was accepted");
    a = ok, a.done = nullptr;
    if (!says(rollout_targets_refusal(a, K, N, 0.9f, 0.9f), "done_dev is NULL")) return fail("a NULL done_dev was accepted");
    a = ok, a.value = nullptr;
    if (!says(rollout_targets_refusal(a, K, N, 0.9f, 0.9f), "value_dev is NULL")) return fail("a NULL value_dev was accepted");
    a = ok, a.adv = nullptr;
    if (!says(rollout_targets_refusal(a, K, N, 0.9f, 0.9f), "all NULL")) return fail("a call without an output was accepted");
    for (int o = 0; o < 4; ++o) {  // each output alone is enough
        a = ok, a.adv = nullptr;
        if (o == 0) a.adv = (float*)out;
        if (o == 1) a.ret = (float*)out;
        if (o == 2) a.valid = (uint8_t*)out;
        if (o == 3) a.col = (double*)out;
        if (rollout_targets_refusal(a, K, N, 0.9f, 0.9f)) return fail("a call with one output was refused");
    }
    if (!says(rollout_targets_refusal(ok, 0, N, 0.9f, 0.9f), "steps < 1") || !says(rollout_targets_refusal(ok, -4, N, 0.9f, 0.9f), "steps < 1"))
        return fail("steps < 1 was accepted");
    if (!says(rollout_targets_refusal(ok, 3, 1 << 29, 0.9f, 0.9f), "INT32_MAX") || !says(rollout_targets_refusal(ok, INT32_MAX, 2, 0.9f, 0.9f), "INT32_MAX"))
        return fail("the int32 limit of (steps + 1) * num_envs");
    if (!says(rollout_targets_refusal(ok, K, N, -0.1f, 0.9f), "gamma") || !says(rollout_targets_refusal(ok, K, N, 1.0001f, 0.9f), "gamma") ||
        !says(rollout_targets_refusal(ok, K, N, nan, 0.9f), "gamma") || !says(rollout_targets_refusal(ok, K, N, 0.9f, -1.0f), "lambda") ||
        !says(rollout_targets_refusal(ok, K, N, 0.9f, 2.0f), "lambda") || !says(rollout_targets_refusal(ok, K, N, 0.9f, nan), "lambda"))
        return fail("a gamma or lambda outside [0, 1] was accepted");
    a = ok, a.final_value = (const float*)(in + 4096);
    if (!says(rollout_targets_refusal(a, K, N, 0.9f, 0.9f), "final_value_dev without trunc_dev")) return fail("final_value_dev without trunc_dev was accepted");
    a.trunc = (const uint8_t*)(in + 8192);
    if (rollout_targets_refusal(a, K, N, 0.9f, 0.9f)) return fail("final_value_dev with trunc_dev was refused");

    // the overlap check: an output range against every input range, byte by byte at the edges
    a = ok, a.adv = (float*)(in + 239);  // the last byte of reward
    if (!says(rollout_targets_refusal(a, K, N, 0.9f, 0.9f), "adv_dev and reward_dev overlap")) return fail("adv on reward's last byte");
    a.adv = (float*)(in + 240);
    if (rollout_targets_refusal(a, K, N, 0.9f, 0.9f)) return fail("adv right behind reward was refused");
    a = ok, a.adv = nullptr, a.valid = (uint8_t*)(in + 1024 + 59);  // done is 60 bytes
    if (!says(rollout_targets_refusal(a, K, N, 0.9f, 0.9f), "valid_dev and done_dev overlap")) return fail("valid on done's last byte");
    a.valid = (uint8_t*)(in + 1024 + 60);
    if (rollout_targets_refusal(a, K, N, 0.9f, 0.9f)) return fail("valid right behind done was refused");
    a.valid = (uint8_t*)(in + 1024 - 60);
    if (rollout_targets_refusal(a, K, N, 0.9f, 0.9f)) return fail("valid right in front of done was refused");
    a.valid = (uint8_t*)(in + 1024 - 59);
    if (!says(rollout_targets_refusal(a, K, N, 0.9f, 0.9f), "valid_dev and done_dev overlap")) return fail("valid's last byte on done");
    a = ok, a.ret = (float*)(in + 2048 + 276);  // value is 280 bytes: the bootstrap row counts
    if (!says(rollout_targets_refusal(a, K, N, 0.9f, 0.9f), "ret_dev and value_dev overlap")) return fail("ret on value's bootstrap row");
    a.ret = (float*)(in + 2048 + 280);
    if (rollout_targets_refusal(a, K, N, 0.9f, 0.9f)) return fail("ret right behind value was refused");
    a = ok, a.col = (double*)(in + 2048 - 232);  // col is 240 bytes
    if (!says(rollout_targets_refusal(a, K, N, 0.9f, 0.9f), "col_dev and value_dev overlap")) return fail("col's last bytes on value");
    a = ok, a.steps_of = (const int32_t*)(out + 236);  // 40 bytes behind adv's 240
    if (!says(rollout_targets_refusal(a, K, N, 0.9f, 0.9f), "adv_dev and steps_of_dev overlap")) return fail("steps_of on adv");
    a = ok, a.skip = (const uint8_t*)out;
    if (!says(rollout_targets_refusal(a, K, N, 0.9f, 0.9f), "adv_dev and skip_dev overlap")) return fail("skip on adv");
    a = ok, a.trunc = (const uint8_t*)(out + 100);
    if (!says(rollout_targets_refusal(a, K, N, 0.9f, 0.9f), "adv_dev and trunc_dev overlap")) return fail("trunc on adv");
    a.final_value = (const float*)(out + 4096), a.ret = (float*)(out + 4096 + 236);
    a.trunc = (const uint8_t*)(in + 8192);
    if (!says(rollout_targets_refusal(a, K, N, 0.9f, 0.9f), "ret_dev and final_value_dev overlap")) return fail("ret on final_value");
    a = ok, a.ret = (float*)(out + 200);
    if (!says(rollout_targets_refusal(a, K, N, 0.9f, 0.9f), "adv_dev and ret_dev overlap")) return fail("two outputs on one another");

    // mg_sum_columns
    if (sum_columns_refusal(in, 1, out) || sum_columns_refusal(in, 3, out)) return fail("a legal sum was refused");
    if (!says(sum_columns_refusal(nullptr, 3, out), "col_dev") || !says(sum_columns_refusal(in, 3, nullptr), "out_dev") || !says(sum_columns_refusal(in, 0, out), "rows < 1"))
        return fail("sum: a NULL buffer or rows < 1 was accepted");
    {  // (its order is held against the definition's bits by the cases file; here: sizes around the 256 partial sums)
        double row[600];
        for (int i = 0; i < 600; ++i) row[i] = (double)(i + 1);
        if (sum_columns_row(row, 1) != 1.0 || sum_columns_row(row, 255) != 32640.0 || sum_columns_row(row, 256) != 32896.0 || sum_columns_row(row, 257) != 33153.0 ||
            sum_columns_row(row, 600) != 180300.0)
            return fail("a sum of small integers");
    }

    if (argc > 1 && run_cases(argv[1])) return 1;
    printf("OK\n");
    return 0;
}
