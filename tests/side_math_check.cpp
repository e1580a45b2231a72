// side_math_check.cpp -- a CPU driver of csrc/agt_side_math.h and csrc/agt_side_frames.h, the host code the side libraries share.  tests/test_side_math.py builds it
// with the host compiler under AddressSanitizer and UBSan, runs it and holds what it prints to its expectations.
//   lm MAX_ITERS FTOL LAMBDA0 UP DOWN LAMBDA_MAX COST0 N_RESIDUALS TRIAL...
//                       lm_options ("-" keeps a default), then lm_solve with callables that replay the trial costs (the last one repeats;
//                       "u": the step is not solved, "f": it fails) -> "rc steps commits", the report, the lambda of every step
//   chol FILE           FILE: int32 n, n x n doubles A (row-major), n doubles b -> "ok" or "refused", then x
//   tilt TAU_X TAU_Y    the 18 doubles of tilt_matrices
//   frames P PITCH FRAME_STRIDE WIDTH HEIGHT CHANNELS B MIN_SIZE MAX_W MAX_H MAX_B
//                       frames_ok with P = 0 for a null pointer, anything else for some address (never read) -> "1" or "0"
// Doubles are printed as %a.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include "../accurate_aprilgroup_tracking_amd/csrc/agt_side_frames.h"
#include "../accurate_aprilgroup_tracking_amd/csrc/agt_side_math.h"
#include "../include/agt_calib.h"

static_assert(AGT_CALIB_OK == agt_side::OK && AGT_CALIB_ERR_ARG == agt_side::ERR_ARG && AGT_CALIB_STOP_CONVERGED == agt_side::STOP_CONVERGED &&
              AGT_CALIB_STOP_MAX_ITERS == agt_side::STOP_MAX_ITERS && AGT_CALIB_STOP_LAMBDA == agt_side::STOP_LAMBDA, "");

static int lm(int argc, char** argv)
{
    agt_calib_options given, o;
    agt_side::lm_default_options(&given);
    double* field[] = { nullptr, &given.ftol, &given.lambda0, &given.lambda_up, &given.lambda_down, &given.lambda_max };
    if (std::string(argv[2]) != "-") given.max_iters = atoi(argv[2]);
    for (int i = 1; i < 6; i++) if (std::string(argv[2 + i]) != "-") *field[i] = strtod(argv[2 + i], nullptr);
    if (!agt_side::lm_options(&given, o)) { printf("%d 0 0\n", AGT_CALIB_ERR_ARG); return 0; }
    int steps = 0, commits = 0;
    std::vector<double> lambdas;
    agt_calib_report rep;
    const int rc = agt_side::lm_solve(o, strtod(argv[8], nullptr), atoi(argv[9]),
        [&](double lambda, double& cost_trial) {
            const std::string t = argv[10 + steps < argc ? 10 + steps : argc - 1];
            steps++;
            lambdas.push_back(lambda);
            if (t == "f") return (int)agt_side::ERR_HIP;
            if (cost_trial != INFINITY) abort();
            if (t != "u") cost_trial = strtod(t.c_str(), nullptr);
            return (int)agt_side::OK;
        },
        [&] { commits++; }, &rep);
    printf("%d %d %d\n", rc, steps, commits);
    if (rc) return 0;
    printf("%d %d %d %d %a %a %a %a\n", rep.iterations, rep.accepted, rep.stop_reason, rep.n_residuals, rep.initial_cost, rep.final_cost,
           rep.final_rms_px, rep.final_lambda);
    for (double l : lambdas) printf("%a ", l);
    printf("\n");
    return 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "lm" && argc >= 11) return lm(argc, argv);
    if (mode == "chol" && argc == 3) {
        FILE* f = fopen(argv[2], "rb");
        int32_t n = 0;
        if (!f || fread(&n, sizeof(n), 1, f) != 1 || n < 0) return 2;
        std::vector<double> A((size_t)n * n), b(n);
        if (fread(A.data(), sizeof(double), A.size(), f) != A.size() || fread(b.data(), sizeof(double), b.size(), f) != b.size()) return 2;
        fclose(f);
        printf(agt_side::cholesky_solve(A, b, n) ? "ok\n" : "refused\n");
        for (double x : b) printf("%a\n", x);
        return 0;
    }
    if (mode == "tilt" && argc == 4) {
        double m[18];
        agt_side::tilt_matrices(strtod(argv[2], nullptr), strtod(argv[3], nullptr), m);
        for (double x : m) printf("%a\n", x);
        return 0;
    }
    if (mode == "frames" && argc == 13) {
        static const uint8_t somewhere = 0;
        long long v[11];
        for (int i = 0; i < 11; i++) v[i] = strtoll(argv[2 + i], nullptr, 10);
        printf("%d\n", (int)agt_side::frames_ok(v[0] ? &somewhere : nullptr, (size_t)v[1], (size_t)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[6],
                                                (int)v[7], (int)v[8], (int)v[9], (int)v[10]));
        return 0;
    }
    fprintf(stderr, "usage: side_math_check lm OPTIONS... COST0 N_RESIDUALS TRIAL... | chol FILE | tilt TAU_X TAU_Y | frames ARGUMENTS...\n");
    return 2;
}
