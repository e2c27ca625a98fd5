//! `ida::traits::IdaProblem` (src/traits.rs:12-94: `Residual + Jacobian + Root`) as a [`HostProblem`]: the reference's own
//! problem structs (e.g. src/sample_problems/roberts.rs) run unchanged behind the C ABI's host callbacks
//! (`IDAHIP_HOST_CALLBACK`), one system at a time; LU, triangular solves, norms and the stepper's vectors stay on the device.
//! Feature `ida-problem` (needs the reference's root crate, which upstream ships without a `[package]` section).
//!
//! Experimental, never compiled (see the crate documentation).
use ida::traits::{Jacobian, Residual};
use ndarray::{ArrayView1, ArrayViewMut1, ArrayViewMut2, ShapeBuilder};

use crate::{Ctx, Error, HostProblem};

/// Wraps one problem instance shared by every system of the batch (the reference integrates one `Ida` per problem; an
/// ensemble of different parameter sets uses one adapter per system through `Vec<P>` below).
pub struct IdaProblemAdapter<P> {
    problems: Vec<P>,
}

impl<P> IdaProblemAdapter<P>
where
    P: Residual<Scalar = f64> + Jacobian<Scalar = f64>,
{
    /// The same problem for every system.
    pub fn shared(problem: P) -> Self {
        IdaProblemAdapter { problems: vec![problem] }
    }
    /// `problems[sys]` for system `sys` (a parameter sweep).
    pub fn per_system(problems: Vec<P>) -> Self {
        assert!(!problems.is_empty());
        IdaProblemAdapter { problems }
    }
    fn of(&self, sys: usize) -> &P {
        &self.problems[if self.problems.len() == 1 { 0 } else { sys }]
    }
}

impl<P> HostProblem for IdaProblemAdapter<P>
where
    P: Residual<Scalar = f64> + Jacobian<Scalar = f64>,
{
    /// `Residual::res(tt, yy, yp, rr)` (src/traits.rs:28-37)
    fn res(&self, sys: usize, tt: f64, yy: &[f64], yp: &[f64], resval: &mut [f64]) {
        self.of(sys).res(tt, ArrayView1::from(yy), ArrayView1::from(yp), ArrayViewMut1::from(resval));
    }

    /// `Jacobian::jac(tt, cj, yy, yp, rr, jac)` (src/traits.rs:58-69). The reference indexes `jac[[row, col]]`
    /// (roberts.rs:80-90); the library's matrix is column-major, i.e. Fortran order of an n x n view.
    fn jac(&self, sys: usize, tt: f64, cj: f64, yy: &[f64], yp: &[f64], resvec: &[f64], jac_colmajor: &mut [f64]) {
        let n = yy.len();
        let j = ArrayViewMut2::from_shape((n, n).f(), jac_colmajor).expect("n x n Jacobian");
        self.of(sys).jac(tt, cj, ArrayView1::from(yy), ArrayView1::from(yp), ArrayView1::from(resvec), j);
    }
}

/// A mass-action reaction network (`Problem::MassAction`, include/ida_hip.h): the tables `Ctx::set_mass_action` takes, built one
/// reaction at a time. Entries are numbered in the order they are added, so within a row they keep that order. A reaction may carry
/// rate-law factors (`factor`: Michaelis-Menten and Hill terms over `constants` per-system constants); the network then goes up
/// through `Ctx::set_rate_network`, and a system's parameters are its rate constants followed by its constants.
pub struct MassAction {
    n: usize,
    nconst: usize,
    factors: Vec<i32>,
    reactants: Vec<i32>,
    rows: Vec<i32>,
    reacs: Vec<i32>,
    nu: Vec<f64>,
    d: Vec<f64>,
}

impl MassAction {
    /// `n` unknowns, every row differential (d = 1.0) and no reaction yet.
    pub fn new(n: usize) -> Self {
        MassAction { n, nconst: 0, factors: Vec::new(), reactants: Vec::new(), rows: Vec::new(), reacs: Vec::new(), nu: Vec::new(), d: vec![1.0; n] }
    }
    /// Reaction of order `reactants.len()` <= 3 (a species may repeat: y1^2 is `&[1, 1]`) with the stoichiometric coefficient `nu`
    /// in each `(row, nu)` of `stoich`. Returns the reaction's index: the position of its rate constant in a system's parameters.
    pub fn reaction(&mut self, reactants: &[usize], stoich: &[(usize, f64)]) -> usize {
        assert!(reactants.len() <= 3 && reactants.iter().all(|&s| s < self.n));
        let r = self.reactants.len() / 3;
        for p in 0..3 {
            self.reactants.push(if p < reactants.len() { reactants[p] as i32 } else { -1 });
        }
        for &(row, nu) in stoich {
            assert!(row < self.n && nu.is_finite());
            self.rows.push(row as i32);
            self.reacs.push(r as i32);
            self.nu.push(nu);
        }
        r
    }
    /// `nconst` constants K per system (they follow the rate constants in a system's parameters) for the factors to name.
    pub fn constants(&mut self, nconst: usize) -> &mut Self {
        self.nconst = nconst;
        self
    }
    /// A factor of reaction `reaction`, after those it already has (at most 4): `RateLaw::Sat` is y^h / (K^h + y^h), `RateLaw::Inh` is
    /// K^h / (K^h + y^h), with y = `species`, K = constant number `constant`, and the exponent 1 <= `h` <= 4.
    pub fn factor(&mut self, reaction: usize, law: RateLaw, species: usize, constant: usize, h: u32) -> &mut Self {
        assert!(reaction < self.nreac() && species < self.n && constant < self.nconst && (1..=4).contains(&h));
        assert!(self.factors.chunks(5).filter(|f| f[0] as usize == reaction).count() < 4);
        let op: i32 = match law {
            RateLaw::Sat => 1, // IDAHIP_RATE_SAT
            RateLaw::Inh => 2, // IDAHIP_RATE_INH
        };
        self.factors.extend_from_slice(&[reaction as i32, op, species as i32, constant as i32, h as i32]);
        self
    }
    /// Parameters per system: the rate constants, then the constants.
    pub fn nparam(&self) -> usize {
        self.nreac() + self.nconst
    }
    /// Row `row` is algebraic: d = 0.0 (a conservation law written as entries that sum to zero).
    pub fn algebraic(&mut self, row: usize) -> &mut Self {
        self.d[row] = 0.0;
        self
    }
    /// Reactions added so far: the number of rate constants per system.
    pub fn nreac(&self) -> usize {
        self.reactants.len() / 3
    }
    /// Uploads the network to a `Problem::MassAction` context.
    pub fn apply(&self, ctx: &mut Ctx) -> Result<(), Error> {
        if self.factors.is_empty() && self.nconst == 0 {
            return ctx.set_mass_action(&self.reactants, &self.rows, &self.reacs, &self.nu, &self.d);
        }
        ctx.set_rate_network(&self.reactants, &self.factors, self.nconst, &self.rows, &self.reacs, &self.nu, &self.d)
    }
}

/// The rate laws a reaction's factor can be (include/ida_hip.h, IDAHIP_RATE_SAT / IDAHIP_RATE_INH).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum RateLaw {
    /// y^h / (K^h + y^h): Michaelis-Menten at h = 1, an activating Hill term above
    Sat,
    /// K^h / (K^h + y^h): inhibition
    Inh,
}
