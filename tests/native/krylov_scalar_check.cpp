// Stand-alone host check of rust-ida_amd/host/krylov_scalar.hpp (tests/test_krylov_scalar.py): runs the scalar part of the SPGMR solver
// on Hessenberg columns dumped from tests/krylov_ref.py and prints the bits of what it computes. Input on stdin, numbers as C99 hex
// floats:
//   S <beta> <tol> <maxl>            a solve begins
//   C <l> <h_0> ... <h_{l+1}>        column l before the Givens update: the Gram-Schmidt coefficients and hn
//   E                                the solve ends: rotation of g, back-substitution
// Output per solve: "flag krydim nli rho | g_0 .. g_{krydim-1} | q_0 .. q_{2 krydim - 1}".
// Also the program to run under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "krylov_scalar.hpp"

int main() {
    static idakry::Sys k;
    char line[8192];
    int maxl = 0;
    bool open = false, ended = false;
    while (std::fgets(line, sizeof line, stdin)) {
        std::vector<std::string> tok;
        for (char* p = std::strtok(line, " \t\r\n"); p; p = std::strtok(nullptr, " \t\r\n")) tok.emplace_back(p);
        if (tok.empty()) continue;
        if (tok[0] == "S" && tok.size() == 4) {
            const double beta = std::strtod(tok[1].c_str(), nullptr), tol = std::strtod(tok[2].c_str(), nullptr);
            maxl = std::atoi(tok[3].c_str());
            if (maxl < 1 || maxl > idakry::MAXL_MAX) return 2;
            ended = idakry::begin(k, beta, tol);
            open = true;
        } else if (tok[0] == "C" && open && tok.size() >= 2) {
            const int l = std::atoi(tok[1].c_str());
            if (ended || l < 0 || l >= maxl || (int)tok.size() != l + 4) return 3;
            for (int i = 0; i <= l + 1; ++i) k.H[i][l] = std::strtod(tok[2 + i].c_str(), nullptr);
            k.nli += 1;
            k.l = l;
            if (idakry::givens_column(k, l)) ended = true;
            else if (l + 1 == maxl) {
                idakry::end_unconverged(k, maxl);
                ended = true;
            }
        } else if (tok[0] == "E" && open) {
            if (!ended) return 4;
            const int flag = idakry::qr_solve(k);
            const bool formed = (flag == idakry::SUCCESS || flag == idakry::RES_REDUCED) && k.krydim > 0;
            std::printf("%d %d %d %a |", flag, k.krydim, k.nli, k.rho);
            for (int i = 0; formed && i < k.krydim; ++i) std::printf(" %a", k.g[i]);
            std::printf(" |");
            for (int i = 0; i < 2 * k.krydim; ++i) std::printf(" %a", k.q[i]);
            std::printf("\n");
            open = false;
        } else {
            return 5;
        }
    }
    std::printf("tol %a sigma %a\n", idakry::tolerance(300, 0.33), idakry::dq_sigma(300));
    return 0;
}
