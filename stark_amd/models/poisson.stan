// Bayesian Poisson (count) regression with a log link, flat priors.
data {
  int<lower=0> N;
  int<lower=0> K;
  matrix[N, K] x;
  int<lower=0> y[N];
}
parameters {
  real alpha;
  vector[K] beta;
}
model {
  y ~ poisson_log(alpha + x * beta);
}
