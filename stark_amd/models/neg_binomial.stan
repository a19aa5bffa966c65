// Bayesian negative-binomial (overdispersed count) regression, log link, flat priors.
// The flat program is what Stan runs too; its posterior is improper in phi (see DESIGN.md section 3).
data {
  int<lower=0> N;
  int<lower=0> K;
  matrix[N, K] x;
  int<lower=0> y[N];
}
parameters {
  real alpha;
  vector[K] beta;
  real<lower=0> phi;
}
model {
  y ~ neg_binomial_2_log(alpha + x * beta, phi);
}
