// nmpf_driver -- closed-loop fleet driver: the openKITE simulator node
// (src/kite_model/simulator.cpp, 50 Hz RK4 plant) and the NMPC node
// (src/kite_control/nmpf_node.cpp: closest-point initialisation, delay
// compensation, minimal-speed clamp, computeControl, mpc_diagnostic publish)
// for B kites at once, on the C ABI of libkite_nmpc.so.  Replaces the ROS
// plumbing; emits the mpc_diagnostic stream (msg/mpc_diagnostic.msg) as JSONL.
//
//   nmpf_driver [--params yaml] [--batch B] [--steps S] [--x0 file.csv]
//               [--ctrl-every K] [--sim-dt h] [--delay d] [--trace T] [--seed s]
//               [--out file.jsonl] [--device i]
//               [--plant-params file.csv] [--plant-wind file.csv]
//               [--plant-delay SECONDS [--plant-delay-dev SECONDS] [--plant-delay-seed S]
//                [--plant-delay-rule sequential|transport] [--delay-comp last|queue]]
//
// --plant-params (B rows of the 52 kite_params values) and --plant-wind (B rows
// of [W0 (3) | A (3) | f_hz | phase]) give every kite a plant of its own, which
// the controller is not told about (kite_nmpc_plant_set_params / _set_wind).
// With either, the plant phase is one kite_nmpc_plant_step call per control
// step (K plant steps of sim-dt inside one kernel) and the summary line gains
// "plant_nan", the kites whose plant state went non-finite on the way to this
// step's measurement.
//
// --plant-delay puts every kite's plant behind a command line (the reference's
// transport_delay node): u(t0) is sent at t0 and arrives after a latency drawn
// per kite and step, uniform on [max(d - dev, 0), d + dev] (seeded), no sooner
// than the command before it; the plant flies what has arrived, at its ticks.
// The plant phase is then one kite_nmpc_plant_step_delayed call per control
// step, with or without --plant-params / --plant-wind, and the summary line
// gains "cmd_dropped", the kites whose full line dropped its oldest command in
// the period before this step's measurement.  --delay is the controller's
// assumption, --plant-delay is the plant's truth.  --plant-delay-rule chooses
// the line's arrival rule (kite_nmpc.h, KITE_DELAY_RULE_*): sequential (the
// default) charges every command its latency after the one before it,
// transport is a pure transport delay that never reorders.  --delay-comp queue
// (it needs --plant-delay) hands the lines to the controller before every step
// (kite_nmpc_set_inflight): the delay compensation then predicts under the
// commands still in flight, not under the last u(t0) alone (last, the default).
//
// Timeline (per control step, all kites in lockstep):
//   measure x (13 plant states) -> kite_nmpc_step (prologue predicts over
//   `delay` when warm) -> u(t0) applied to the plant for K plant steps of
//   sim-dt (kite_nmpc_predict, RK4 with 4 substeps per plant step, the
//   simulator's integrator).  Per step one summary line; per traced kite one
//   mpc_diagnostic line.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "kite_nmpc/kite_nmpc.h"

namespace {

struct Args {
    std::string params = "data/umx_radian.yaml";
    std::string x0_file, out_file, plant_params_file, plant_wind_file;
    int batch = 64, steps = 100, ctrl_every = 3, trace = 1, device = 0;
    double sim_dt = 0.02, delay = 0.1;
    double plant_delay = -1.0, plant_delay_dev = 0.0;      // < 0: no command line
    unsigned long long seed = 20261015ull, plant_delay_seed = 0ull;
    int plant_delay_rule = KITE_DELAY_RULE_SEQUENTIAL;
    bool comp_queue = false;
};

[[noreturn]] void usage(const char* argv0) {
    std::fprintf(stderr,
                 "usage: %s [--params yaml] [--batch B] [--steps S] [--x0 file.csv] [--ctrl-every K]\n"
                 "          [--sim-dt h] [--delay d] [--trace T] [--seed s] [--out file.jsonl] [--device i]\n"
                 "          [--plant-params file.csv] [--plant-wind file.csv]\n"
                 "          [--plant-delay seconds [--plant-delay-dev seconds] [--plant-delay-seed S]\n"
                 "           [--plant-delay-rule sequential|transport] [--delay-comp last|queue]]\n",
                 argv0);
    std::exit(2);
}

Args parse(int argc, char** argv) {
    Args a;
    for (int i = 1; i < argc; ++i) {
        const std::string k = argv[i];
        auto val = [&]() -> const char* {
            if (i + 1 >= argc) usage(argv[0]);
            return argv[++i];
        };
        if (k == "--params") a.params = val();
        else if (k == "--batch") a.batch = std::atoi(val());
        else if (k == "--steps") a.steps = std::atoi(val());
        else if (k == "--x0") a.x0_file = val();
        else if (k == "--ctrl-every") a.ctrl_every = std::atoi(val());
        else if (k == "--sim-dt") a.sim_dt = std::atof(val());
        else if (k == "--delay") a.delay = std::atof(val());
        else if (k == "--trace") a.trace = std::atoi(val());
        else if (k == "--seed") a.seed = std::strtoull(val(), nullptr, 10);
        else if (k == "--out") a.out_file = val();
        else if (k == "--device") a.device = std::atoi(val());
        else if (k == "--plant-params") a.plant_params_file = val();
        else if (k == "--plant-wind") a.plant_wind_file = val();
        else if (k == "--plant-delay") { a.plant_delay = std::atof(val()); if (!(a.plant_delay >= 0)) usage(argv[0]); }
        else if (k == "--plant-delay-dev") a.plant_delay_dev = std::atof(val());
        else if (k == "--plant-delay-seed") a.plant_delay_seed = std::strtoull(val(), nullptr, 10);
        else if (k == "--plant-delay-rule") {
            const std::string v = val();
            if (v == "transport") a.plant_delay_rule = KITE_DELAY_RULE_TRANSPORT;
            else if (v == "sequential") a.plant_delay_rule = KITE_DELAY_RULE_SEQUENTIAL;
            else usage(argv[0]);
        } else if (k == "--delay-comp") {
            const std::string v = val();
            if (v == "queue") a.comp_queue = true;
            else if (v == "last") a.comp_queue = false;
            else usage(argv[0]);
        }
        else usage(argv[0]);
    }
    if (a.comp_queue && !(a.plant_delay >= 0.0)) usage(argv[0]);      // there is no line to look at
    if (!std::isfinite(a.plant_delay) || !(a.plant_delay_dev >= 0) || !std::isfinite(a.plant_delay_dev)) usage(argv[0]);
    if (a.batch < 1 || a.steps < 0 || a.ctrl_every < 1 || !(a.sim_dt > 0) || a.trace < 0) usage(argv[0]);
    return a;
}

// launch/simulator.launch:3 initial state, perturbed per kite (seeded)
void synthetic_states(int B, unsigned long long seed, std::vector<double>& x) {
    const double base[13] = {4.4, 0.44, 1.73, 0.81, -1.73, -1.53, -0.46, -2.68, 0.64,
                             -0.0289, 0.1587, 0.4304, 0.8881};
    x.assign((size_t)B * 13, 0.0);
    for (int b = 0; b < B; ++b) {
        std::mt19937_64 rng(seed + (unsigned long long)b);
        std::uniform_real_distribution<double> U(-1.0, 1.0);
        double* s = &x[(size_t)b * 13];
        for (int i = 0; i < 13; ++i) s[i] = base[i];
        for (int i = 0; i < 3; ++i) s[i] += 0.5 * U(rng);
        for (int i = 3; i < 6; ++i) s[i] += 0.3 * U(rng);
        for (int i = 6; i < 9; ++i) s[i] += 0.05 * U(rng);
        double n = 0;
        for (int i = 9; i < 13; ++i) { s[i] += 0.02 * U(rng); n += s[i] * s[i]; }
        n = std::sqrt(n);
        for (int i = 9; i < 13; ++i) s[i] /= n;
    }
}

bool read_csv(const std::string& path, int B, std::vector<double>& x, int cols = 13) {
    FILE* f = std::fopen(path.c_str(), "r");
    if (!f) return false;
    x.assign((size_t)B * cols, 0.0);
    for (size_t i = 0; i < x.size(); ++i) {
        if (std::fscanf(f, " %lf ,", &x[i]) != 1) { std::fclose(f); return false; }
    }
    std::fclose(f);
    return true;
}

int fail(const char* what, int rc) {
    std::fprintf(stderr, "nmpf_driver: %s: %s (%d)\n", what, kite_nmpc_strerror(rc), rc);
    return 1;
}

// %.17g that stays valid JSON (NaN / inf -> null)
void jnum(FILE* f, double v, const char* sep) {
    if (std::isfinite(v)) std::fprintf(f, "%.17g%s", v, sep);
    else std::fprintf(f, "null%s", sep);
}

}  // namespace

int main(int argc, char** argv) {
    const Args a = parse(argc, argv);
    const int B = a.batch;
    kite_params kp;
    int rc = kite_params_load_yaml(a.params.c_str(), &kp);
    if (rc) return fail("load params", rc);
    kite_nmpc_config cfg;
    kite_nmpc_default_config(&cfg);
    cfg.device = a.device;
    cfg.delay = a.delay;                  // node: 0.1 s (nmpf_node.cpp:74)
    kite_nmpc_ctx* ctx = nullptr;
    rc = kite_nmpc_create(&kp, &cfg, B, &ctx);
    if (rc) return fail("create", rc);

    // a plant of its own (model, wind, gust per kite) instead of the controller's model
    const bool own_plant = !a.plant_params_file.empty() || !a.plant_wind_file.empty();
    if (!a.plant_params_file.empty()) {
        static_assert(sizeof(kite_params) == 52 * sizeof(double), "kite_params holds 52 doubles");
        std::vector<double> pp;
        if (!read_csv(a.plant_params_file, B, pp, 52)) {
            std::fprintf(stderr, "nmpf_driver: cannot read %s\n", a.plant_params_file.c_str());
            return 1;
        }
        std::vector<kite_params> kps(B);
        std::memcpy(kps.data(), pp.data(), pp.size() * sizeof(double));
        rc = kite_nmpc_plant_set_params(ctx, kps.data(), B);
        if (rc) return fail("plant params", rc);
    }
    if (!a.plant_wind_file.empty()) {
        std::vector<double> pw;
        if (!read_csv(a.plant_wind_file, B, pw, 8)) {
            std::fprintf(stderr, "nmpf_driver: cannot read %s\n", a.plant_wind_file.c_str());
            return 1;
        }
        rc = kite_nmpc_plant_set_wind(ctx, pw.data());
        if (rc) return fail("plant wind", rc);
    }
    std::vector<int32_t> plant_status(B, 0);
    // a command line per kite (all zero: empty, zero control in force) and its latencies
    const bool delayed = a.plant_delay >= 0.0;
    std::vector<double> line, tau, u_applied;
    std::mt19937_64 tau_rng(a.plant_delay_seed);
    std::uniform_real_distribution<double> tau_dist(std::fmax(a.plant_delay - a.plant_delay_dev, 0.0),
                                                    a.plant_delay + a.plant_delay_dev);
    if (delayed) {
        line.assign((size_t)B * KITE_DELAY_NLINE, 0.0);
        for (int b = 0; b < B; ++b) line[(size_t)b * KITE_DELAY_NLINE + KITE_DELAY_RULE] = (double)a.plant_delay_rule;
        tau.assign((size_t)B, a.plant_delay);
        u_applied.assign((size_t)B * 4, 0.0);
    }

    std::vector<double> plant;            // B x 13 plant states
    if (!a.x0_file.empty()) {
        if (!read_csv(a.x0_file, B, plant)) { std::fprintf(stderr, "nmpf_driver: cannot read %s\n", a.x0_file.c_str()); return 1; }
    } else {
        synthetic_states(B, a.seed, plant);
    }
    FILE* out = a.out_file.empty() ? stdout : std::fopen(a.out_file.c_str(), "w");
    if (!out) { std::fprintf(stderr, "nmpf_driver: cannot open %s\n", a.out_file.c_str()); return 1; }

    const int N = cfg.N;
    std::vector<double> x0((size_t)B * 15), u0((size_t)B * 4), traj((size_t)B * (N + 1) * 15);
    std::vector<double> pos((size_t)B * 3), guess((size_t)B, 0.0), theta((size_t)B), x15((size_t)B * 15),
        u4((size_t)B * 4, 0.0), xn((size_t)B * 15);
    std::vector<kite_mpc_diagnostic> diag(B);
    std::vector<int32_t> status(B);

    // initialisation (nmpf_node.cpp:233-236): closest point, thetadot = 0
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < 3; ++i) pos[(size_t)b * 3 + i] = plant[(size_t)b * 13 + 6 + i];
    rc = kite_nmpc_closest_point(ctx, B, pos.data(), guess.data(), theta.data());
    if (rc) return fail("closest point", rc);

    double t = 0.0;
    for (int s = 0; s < a.steps; ++s) {
        // measurement: plant state; theta/thetadot only matter on the cold step
        // (warm steps take them from the previous plan, nmpf_node.cpp:220)
        for (int b = 0; b < B; ++b) {
            double* xb = &x0[(size_t)b * 15];
            std::memcpy(xb, &plant[(size_t)b * 13], 13 * sizeof(double));
            xb[13] = s == 0 ? theta[b] : traj[(size_t)b * (N + 1) * 15 + 15 + 13];
            xb[14] = s == 0 ? 0.0 : traj[(size_t)b * (N + 1) * 15 + 15 + 14];
        }
        if (a.comp_queue) {
            // the lines as they stand at the measurement: what is in flight
            rc = kite_nmpc_set_inflight(ctx, line.data(), t);
            if (rc) return fail("in-flight schedule", rc);
        }
        const auto c0 = std::chrono::steady_clock::now();
        rc = kite_nmpc_step(ctx, x0.data(), u0.data(), traj.data(), nullptr, diag.data(), status.data());
        if (rc) return fail("step", rc);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();

        // publish: summary + traced kites' mpc_diagnostic records
        double pe_sum = 0, pe_max = 0, ve_sum = 0, th_sum = 0;
        int n_rej = 0, n_nan = 0, n_nc = 0, n_rst = 0;
        int n_fin = 0;
        for (int b = 0; b < B; ++b) {
            if (std::isfinite(diag[b].pos_error) && std::isfinite(diag[b].vel_error) && std::isfinite(diag[b].virt_state)) {
                pe_sum += diag[b].pos_error; pe_max = std::fmax(pe_max, diag[b].pos_error);
                ve_sum += diag[b].vel_error; th_sum += diag[b].virt_state;
                ++n_fin;
            }
            n_nan += (status[b] & KITE_ST_NAN) != 0;
            n_nc += (status[b] & KITE_ST_QP_NOT_CONV) != 0;
            n_rej += (status[b] & KITE_ST_STEP_REJECTED) != 0;
            n_rst += (status[b] & KITE_ST_RESTART) != 0;
        }
        // aggregates over the finite kites only (a NaN kite restarts next step)
        std::fprintf(out,
                     "{\"type\": \"step\", \"step\": %d, \"t\": %.4f, \"comp_time_ms\": %.4f, \"pos_error_mean\": %.9g, "
                     "\"pos_error_max\": %.9g, \"vel_error_mean\": %.9g, \"virt_state_mean\": %.9g, \"nan\": %d, "
                     "\"qp_not_converged\": %d, \"step_rejected\": %d, \"restarts\": %d",
                     s, t, ms, pe_sum / std::max(1, n_fin), pe_max, ve_sum / std::max(1, n_fin),
                     th_sum / std::max(1, n_fin), n_nan, n_nc, n_rej, n_rst);
        if (own_plant) {
            int n_pnan = 0;
            for (int b = 0; b < B; ++b) n_pnan += (plant_status[b] & KITE_PLANT_NAN) != 0;
            std::fprintf(out, ", \"plant_nan\": %d", n_pnan);
        }
        if (delayed) {
            int n_drop = 0;
            for (int b = 0; b < B; ++b) n_drop += (plant_status[b] & KITE_PLANT_CMD_DROPPED) != 0;
            std::fprintf(out, ", \"cmd_dropped\": %d", n_drop);
        }
        std::fprintf(out, "}\n");
        for (int b = 0; b < std::min(a.trace, B); ++b) {
            const double* ub = &u0[(size_t)b * 4];
            std::fprintf(out, "{\"type\": \"mpc_diagnostic\", \"kite\": %d, \"step\": %d, \"pos_error\": ", b, s);
            jnum(out, diag[b].pos_error, ", \"vel_error\": ");
            jnum(out, diag[b].vel_error, ", \"cost\": ");
            jnum(out, diag[b].cost, ", \"virt_state\": ");
            jnum(out, diag[b].virt_state, ", \"virt_ctrl\": ");
            jnum(out, diag[b].virt_ctrl, "");
            std::fprintf(out, ", \"comp_time_ms\": %.4f, \"status\": %d, \"u\": [", ms, status[b]);
            for (int c = 0; c < 4; ++c) jnum(out, ub[c], c < 3 ? ", " : "], \"x\": [");
            for (int i = 0; i < 13; ++i) jnum(out, plant[(size_t)b * 13 + i], i < 12 ? ", " : "]}\n");
        }

        // plant: u(t0) held for ctrl_every simulator steps (simulator.cpp:43-51)
        for (int b = 0; b < B; ++b) {
            std::memcpy(&u4[(size_t)b * 4], &u0[(size_t)b * 4], 3 * sizeof(double));
            u4[(size_t)b * 4 + 3] = 0.0;
        }
        if (delayed) {
            // one launch for the whole control period: u(t0) goes down the line
            if (a.plant_delay_dev > 0.0)
                for (int b = 0; b < B; ++b) tau[b] = tau_dist(tau_rng);
            rc = kite_nmpc_plant_step_delayed(ctx, plant.data(), u4.data(), tau.data(), line.data(), u_applied.data(), t,
                                              a.sim_dt, a.ctrl_every, 4, plant_status.data());
            if (rc) return fail("delayed plant", rc);
            for (int k = 0; k < a.ctrl_every; ++k) t += a.sim_dt;
            continue;
        }
        if (own_plant) {
            // one launch for the whole control period, from the time the step began
            rc = kite_nmpc_plant_step(ctx, plant.data(), u4.data(), t, a.sim_dt, a.ctrl_every, 4, plant_status.data());
            if (rc) return fail("plant", rc);
            for (int k = 0; k < a.ctrl_every; ++k) t += a.sim_dt;
            continue;
        }
        for (int k = 0; k < a.ctrl_every; ++k) {
            for (int b = 0; b < B; ++b) {
                std::memcpy(&x15[(size_t)b * 15], &plant[(size_t)b * 13], 13 * sizeof(double));
                x15[(size_t)b * 15 + 13] = 0.0;
                x15[(size_t)b * 15 + 14] = 0.0;
            }
            rc = kite_nmpc_predict(ctx, B, x15.data(), u4.data(), a.sim_dt, 4, xn.data());
            if (rc) return fail("plant", rc);
            for (int b = 0; b < B; ++b) std::memcpy(&plant[(size_t)b * 13], &xn[(size_t)b * 15], 13 * sizeof(double));
            t += a.sim_dt;
        }
    }
    if (out != stdout) std::fclose(out);
    kite_nmpc_destroy(ctx);
    return 0;
}
